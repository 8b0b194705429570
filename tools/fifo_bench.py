"""Measurements of slot timesteps and FIFO diagonal denoising at the C3 geometry (256 x 256: latent [B, 8, 12, 32, 32], tube 2 x 4 x 4,
384 + 37 tokens), on one GPU, in one process:

  --kernels   the slot form of the fused update and of the assembly pass against their per-sample forms (the per-sample form timed
              twice: its run-to-run spread), and the queue shift kernel with its bytes per microsecond; per-launch times from the
              library's launch events (avd_prof_enable / avd_prof_report)
  --e2e       finished latent slots per second of stream_infer.fifo_denoise (n = 48 steps, S = 6, B = 8) next to the window-consensus
              loop at the same step count, and the share of a steady iteration spent in set_prompt and the shift

  --solver    ddim (default) or dpmpp_2m.  With dpmpp_2m, --kernels times the fused DPM-Solver++(2M) update inside whole steps
              (DenoiseEngine.step against step_slots(t_last=): no entry runs the per-sample CFG form alone) and the queue shift with
              history against the plain one; --e2e runs fifo_denoise on a dpmpp_2m engine at --steps (default 18: the multiple of S = 6
              nearest to 20; ddim: 48) and prints the time per finished slot and the ramp time
  --steps     --e2e: n, the schedule's steps = the queue's slots (a multiple of S = 6)
  --graph     --e2e: fifo_denoise(graph=True) — the iterations replayed from captured HIP graphs, the ramp row, the prompt positions and
              the clip slot read off device cursors — and the cost of the two captures themselves; without it the eager loop

  --lookahead CTX  FIFO lookahead (overlapping windows, CTX held context slots of every window's S = 6).  --kernels: the lookahead
              launch at shift 0 and 1, with and without history, beside the plain shift in the same session, with the bytes it moves
              (every owner read once, B * S slots written); --e2e: fifo_denoise(lookahead=CTX) on B = n / (S - CTX) windows beside the
              plain queue (B = n / S) at the same schedule, time per finished slot and ramp time, on --solver

  --stochastic  eta > 0 on a seeded engine, the step noise keyed by clip position ("clip-keyed slot noise"), both solvers in one session
              (DDIM eta 0.5 at n = 48, dpmpp_2m eta 1.0 at n = 18).  --kernels: the fused update of the seeded slot step inside whole
              2-layer steps, between two runs of the eta = 0 slot step, beside the canvas-keyed and the eta = 0 per-sample steps;
              --e2e: fifo_denoise per finished slot, eager and replayed, the eta = 0 and the eta > 0 engine's calls interleaved

  --guide     the clip-keyed latent guide ("clip-keyed latent guide"), both solvers at eta 0 and eta > 0 in one session.  --kernels: the
              guided fused slot update inside whole 2-layer steps between two runs of the unguided slot update of the same engine, and
              the stand-alone pass (all slots, and the entering tail slot alone, in place) beside the queue shift; --e2e:
              fifo_denoise(init_canvas=) per finished slot beside the unguided queue, eager, the calls interleaved

  --slot-cfg  the slot CFG control ("slot CFG control"), both solvers at eta 0 and eta > 0 in one session.  --kernels: the fused slot
              update inside whole 2-layer steps, plain, under a guidance table alone, under a per-slot rescale (its statistics and
              finalize launches on lines of their own) and under per-slot APG (likewise), between two runs of the plain update;
              --e2e: fifo_denoise per finished slot with and without the control (table + rescale, table + APG), eager, the calls
              interleaved

  --guided-shift  the guided FIFO queue shift ("Guided FIFO queue shift").  --kernels: the guided shift against the plain shift plus the
              in-place guide pass on the tail slot, with and without history, at B = 8 and B = 32, beside the plain shift alone;
              --e2e: fifo_denoise(init_canvas=) per finished slot with guided_shift off (a stand-alone tail pass per shift) and on,
              beside the unguided queue, both solvers, eager, the calls interleaved

Prints plain text: the records are profiles/fifo_kernels.txt and profiles/fifo_e2e.txt (ddim), profiles/fifo_dpm_kernels.txt and
profiles/fifo_dpm_e2e.txt (both solvers in one session), profiles/fifo_graph_e2e.txt (--e2e with and without --graph),
profiles/fifo_lookahead_kernels.txt and profiles/fifo_lookahead_e2e.txt (--lookahead 3), profiles/fifo_stochastic_kernels.txt and
profiles/fifo_stochastic_e2e.txt (--stochastic), profiles/fifo_guide_kernels.txt (--guide), profiles/slot_cfg_kernels.txt and
profiles/slot_cfg_e2e.txt (--slot-cfg), profiles/fifo_guided_shift_kernels.txt and profiles/fifo_guided_shift_e2e.txt (--guided-shift)."""
import argparse
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import multimodal_diffusion_amd as A                       # noqa: E402
from multimodal_diffusion_amd import _lib as L             # noqa: E402
from multimodal_diffusion_amd import functional as Fn      # noqa: E402
from multimodal_diffusion_amd import schedule_utils as su  # noqa: E402
from multimodal_diffusion_amd.stream_infer import fifo_prompt_len, fifo_prompt_windows  # noqa: E402
from oracle import ref_cpu as R                            # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--kernels", action="store_true")
ap.add_argument("--e2e", action="store_true")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--launches", type=int, default=50)
ap.add_argument("--slots-out", type=int, default=24, help="--e2e: finished slots per timed fifo_denoise call")
ap.add_argument("--solver", choices=("ddim", "dpmpp_2m"), default="ddim")
ap.add_argument("--graph", action="store_true", help="--e2e: replay the iterations from captured HIP graphs")
ap.add_argument("--steps", type=int, default=None, help="--e2e: steps of the schedule = slots of the queue (default 48, dpmpp_2m: 18)")
ap.add_argument("--lookahead", type=int, default=0, metavar="CTX", help="FIFO lookahead: CTX context slots per window of S = 6")
ap.add_argument("--stochastic", action="store_true", help="eta > 0 with clip-keyed slot noise beside eta = 0, both solvers")
ap.add_argument("--guide", action="store_true", help="the clip-keyed latent guide beside the unguided slot update and queue")
ap.add_argument("--slot-cfg", action="store_true", help="the slot CFG control beside the plain slot update and queue")
ap.add_argument("--guided-shift", action="store_true", help="the guided queue shift beside the plain shift followed by the tail slot's pass")
args = ap.parse_args()
if not 0 <= args.lookahead < 6:
    raise SystemExit("--lookahead CTX must lie in [0, 6)")
DPM = args.solver == "dpmpp_2m"

dev = torch.device("cuda:0")
ABAR = R.alpha_bar_table(R.beta_table(1000))


def build(n_layers, B, target="video", solver="ddim", **kw):
    ws = R.synth_weights(seed=0, n_layers=n_layers)
    core = A.MMDiT(d_model=512, n_layers=n_layers, n_heads=8, mlp_ratio=4.0).eval()
    core.load_state_dict(ws["core"], strict=True)
    head = A.MultiModalNoiseHead({"video": 512, "audio": 512}, {"video": 256, "audio": 32}, hidden_dim=512).eval()
    head.load_state_dict(ws["head"], strict=True)
    av, aa = A.LinearAdapter(256, 256), A.LinearAdapter(32, 256)
    av.load_state_dict(ws["adapt_v"])
    aa.load_state_dict(ws["adapt_a"])
    core, head, av, aa = (m.to(dev) for m in (core, head, av, aa))
    return A.DenoiseEngine(adapt_v=av, adapt_a=aa, core=core, head=head, tstep_dim=256, target=target,
                           latent_shape=(B, 8, 12, 32, 32), prompt_tokens=37, alpha_bar=ABAR, guidance=3.5, matmul="bf16x3", solver=solver, **kw)


def per_launch_us(tag, fn, launches):
    """mean microseconds per launch of the kernels recorded under `tag` while fn() runs `launches` times"""
    L.prof_enable(True)
    try:
        for _ in range(launches):
            fn()
        torch.cuda.synchronize()
    finally:
        L.prof_enable(False)
    n, ms, _ = L.prof_report()[tag]
    assert n == launches, (tag, n, launches)
    return 1e3 * ms / n


def report_shift(res, cases):
    for name, zz, streams in cases:
        nbytes = 4 * (streams * zz.numel() + zz[0, :, :2].numel())
        us = statistics.median(res[name])
        print(f"  {name}: {nbytes / 1e6:.2f} MB read + written, {nbytes / us / 1e3:.1f} GB/s ({nbytes / us:.0f} bytes per microsecond)")


STOCHASTIC = (("ddim", 0.5, 48), ("dpmpp_2m", 1.0, 18))      # solver, eta, steps: the two queues of profiles/fifo_dpm_e2e.txt

if args.slot_cfg and args.kernels:
    B, S = 32, 6
    g = torch.Generator().manual_seed(0)
    z = torch.randn(B, 8, 12, 32, 32, generator=g).to(dev)
    prompt = torch.randn(B, 8, 150, generator=g).to(dev)
    out = torch.empty_like(z)
    gtab = su.guidance_interval_table(5.0, (200, 800), 1000)
    PLAIN, CTL = "cfg_unpatch_ddim_kernel", "cfg_unpatch_ddim_kernel<slot cfg>"
    STATS, FIN = "slot_cfg_stats_kernel", "slot_cfg_finalize_kernel"
    KINDS = {"plain": None, "table": dict(guidance=gtab), "rescale": dict(guidance=gtab, rescale=0.7),
             "apg": dict(guidance=gtab, apg={"norm_threshold": 20.0, "eta_parallel": 0.5})}
    rows = []
    for solver, eta, n in (("ddim", 0.0, 48), ("ddim", 0.5, 48), ("dpmpp_2m", 0.0, 18), ("dpmpp_2m", 1.0, 18)):
        dpm = solver == "dpmpp_2m"
        sched = su.make_sampling_schedule(1000, n)
        eng = build(2, B, solver=solver, eta=eta, **({"noise_seed": 11} if eta else {}))
        eng.set_prompt(prompt)
        if dpm:
            eng.x0_hist.copy_(torch.randn(B, 8, 12, 32, 32, generator=g))
        i = (torch.arange(B * S) % (n - 2)).view(B, S) + 1      # the diagonal: none held, none final
        tlS, tnS, tpS = (sched[i + d].to(dev).contiguous() for d in (-1, 0, 1))
        last = dict(t_last=tlS) if dpm else {}

        def step(kind, eng=eng, last=last, tnS=tnS, tpS=tpS):
            if KINDS[kind] is None:
                eng.clear_slot_cfg()
            else:
                eng.set_slot_cfg(**KINDS[kind])
            return lambda: eng.step_slots(z, tnS, tpS, out=out, clip_first=0, **last)

        name = f"{solver} eta = {eta}"
        rows += [(f"{name}, plain (a)", PLAIN, step, "plain"), (f"{name}, guidance table", CTL, step, "table"),
                 (f"{name}, rescale: update", CTL, step, "rescale"), (f"{name}, rescale: statistics", STATS, step, "rescale"),
                 (f"{name}, rescale: finalize", FIN, step, "rescale"), (f"{name}, APG: update", CTL, step, "apg"),
                 (f"{name}, APG: statistics", STATS, step, "apg"), (f"{name}, APG: finalize", FIN, step, "apg"),
                 (f"{name}, plain (b)", PLAIN, step, "plain")]
    for _, _, mk, kind in rows:
        fn = mk(kind)
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    res = {name: [] for name, _, _, _ in rows}
    for _ in range(args.rounds):
        for name, tag, mk, kind in rows:
            res[name].append(per_launch_us(tag, mk(kind), args.launches))
    print(f"C3 geometry, B = {B} (S = {S} slots of 16384 elements: 16 chunks per slot): the fused CFG + un-patch + solver slot update inside "
          f"whole steps (2 layers), plain (tag {PLAIN}) and under a slot CFG control (tag {CTL}: a guidance table by level; the table and "
          f"a per-slot rescale phi = 0.7; the table and per-slot APG), with the statistics and finalize launches of the rescale and of APG "
          f"(tags {STATS}, {FIN}): {args.rounds} interleaved rounds of {args.launches} launches, microseconds per launch (launch events)")
    for name, _, _, _ in rows:
        v = res[name]
        print(f"  {name:40s} " + " ".join(f"{x:8.2f}" for x in v) + f"   median {statistics.median(v):8.2f}")
    sys.exit(0)

if args.slot_cfg and args.e2e:
    S, K = 6, args.slots_out
    g = torch.Generator().manual_seed(1)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    gtab = su.guidance_interval_table(5.0, (200, 800), 1000)
    print(f"fifo_denoise plain and under a slot CFG control (guidance by level with a per-slot rescale phi = 0.7, and with per-slot APG), "
          f"S = {S} (C3 latent, 8 layers, bf16x3, eager), {args.rounds} rounds, the calls interleaved, {K} and {2 * K} slots out; milliseconds")
    for solver, eta, n in (("ddim", 0.0, 48), ("dpmpp_2m", 0.0, 18)):
        sched = su.make_sampling_schedule(1000, n)
        canvas_p = torch.randn(8, 25 * (n + 2 * K) + 148, generator=g).to(dev)
        eng = build(8, n // S, solver=solver)
        kinds = [("plain", {}), ("rescale", dict(guidance_by_level=gtab, rescale_by_level=0.7)),
                 ("apg", dict(guidance_by_level=gtab, apg={"norm_threshold": 20.0, "eta_parallel": 0.5}))]
        for _, kw in kinds:
            A.fifo_denoise(eng, canvas_p, 25, sched, 4, 5, **kw)      # warm-up
        ts_ = {(name, K_): [] for name, _ in kinds for K_ in (K, 2 * K)}
        for _ in range(args.rounds):
            for K_ in (K, 2 * K):
                for name, kw in kinds:
                    ts_[name, K_].append(timed(lambda: A.fifo_denoise(eng, canvas_p, 25, sched, K_, 5, **kw)))
        per = {}
        for name, _ in kinds:
            whole = {K_: statistics.median(ts_[name, K_]) for K_ in (K, 2 * K)}
            per[name] = (whole[2 * K] - whole[K]) / K
            print(f"  {solver:8s} n = {n}, B = {n // S}, {name:8s}: " +
                  "; ".join(f"{K_} out " + " ".join(f"{t * 1e3:7.1f}" for t in ts_[name, K_]) for K_ in (K, 2 * K)) +
                  f"; per finished slot {per[name] * 1e3:.3f}, ramp and start {(whole[K] - K * per[name]) * 1e3:.1f}")
        for name in ("rescale", "apg"):
            print(f"  {'':8s} per finished slot, {name} against plain: {(per[name] - per['plain']) * 1e3:+.3f} ms (x {per[name] / per['plain']:.3f})")
    sys.exit(0)

if args.guided_shift and args.kernels:
    S, sl = 6, 2
    g = torch.Generator().manual_seed(0)
    ABAR_D = ABAR.to(dev)
    known = torch.randn(8, 32 * 12 + 2 * sl, 32, 32, generator=g).to(dev)      # the clip under the largest queue and its entering slot
    mask = torch.rand(known.shape, generator=g).to(dev)
    guide = dict(known=known, mask=mask, seed=3, alpha_bar=ABAR_D)
    SHIFT, HIST, PASS = "fifo_shift_kernel<4>", "fifo_shift_kernel<4, HistShift>", "clip_guide_slots_kernel<4>"
    rows = []
    for b in (8, 32):
        zz, hh, ho = (torch.randn(b, 8, 12, 32, 32, generator=g).to(dev) for _ in range(3))
        tail = torch.full((b, S), Fn.SLOT_LEAVE, dtype=torch.long, device=dev)
        tail[b - 1, S - 1] = 999
        c = b * S                                               # the entering clip slot of a queue that holds slots 0 .. b * S - 1
        shift = lambda zz=zz, c=c: Fn.fifo_shift(zz, c, 7, 999, sl)
        shift_h = lambda zz=zz, hh=hh, ho=ho, c=c: Fn.fifo_shift(zz, c, 7, 999, sl, hist=hh, hist_out=ho)
        tail_pass = lambda zz=zz, tail=tail: Fn.clip_guide_slots(known, tail, ABAR_D, zz, mask, first=1, out=zz, slot_len=sl, seed=3)
        rows += [(f"B={b}: plain shift (a)", SHIFT, shift), (f"B={b}: tail slot's guide pass, in place", PASS, tail_pass),
                 (f"B={b}: guided shift", "fifo_shift_kernel<4, GuideShift>", lambda zz=zz, c=c: Fn.fifo_shift(zz, c, 7, 999, sl, guide=guide)),
                 (f"B={b}: plain shift (b)", SHIFT, shift), (f"B={b}: shift with history (a)", HIST, shift_h),
                 (f"B={b}: guided shift with history", "fifo_shift_kernel<4, HistShift, GuideShift>",
                  lambda zz=zz, hh=hh, ho=ho, c=c: Fn.fifo_shift(zz, c, 7, 999, sl, hist=hh, hist_out=ho, guide=guide)),
                 (f"B={b}: shift with history (b)", HIST, shift_h)]
    for _, _, fn in rows:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    res = {name: [] for name, _, _ in rows}
    for _ in range(args.rounds):
        for name, tag, fn in rows:
            res[name].append(per_launch_us(tag, fn, args.launches))
    print(f"C3 geometry (latent [B, 8, 12, 32, 32], S = {S} slots of {sl}), a fractional mask canvas: the guided queue shift against the "
          f"plain shift and the stand-alone guide pass on the entering tail slot (in place), with and without the solver history: "
          f"{args.rounds} interleaved rounds of {args.launches} launches, microseconds per launch (launch events)")
    for name, _, _ in rows:
        v = res[name]
        print(f"  {name:44s} " + " ".join(f"{x:8.2f}" for x in v) + f"   median {statistics.median(v):8.2f}")
    med = {name: statistics.median(v) for name, v in res.items()}
    for b in (8, 32):
        two = med[f"B={b}: plain shift (a)"] + med[f"B={b}: tail slot's guide pass, in place"]
        twoh = med[f"B={b}: shift with history (a)"] + med[f"B={b}: tail slot's guide pass, in place"]
        print(f"  B={b}: shift + tail pass {two:.2f} -> guided shift {med[f'B={b}: guided shift']:.2f}; with history {twoh:.2f} -> "
              f"{med[f'B={b}: guided shift with history']:.2f} (kernel time; the saved launch itself is host time, see --e2e)")
    sys.exit(0)

if args.guided_shift and args.e2e:
    S, K = 6, args.slots_out
    g = torch.Generator().manual_seed(1)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    print(f"fifo_denoise with init_canvas (frames kept on a third of the clip): the entering slot guided by a stand-alone pass after every "
          f"shift (guided_shift=False) and inside the shift's launch (guided_shift=True), beside the unguided queue; S = {S} (C3 latent, "
          f"8 layers, bf16x3, eager), {args.rounds} rounds, the calls interleaved, {K} and {2 * K} slots out; milliseconds")
    for solver, eta, n in (("ddim", 0.0, 48), ("dpmpp_2m", 0.0, 18)):
        sched = su.make_sampling_schedule(1000, n)
        canvas_p = torch.randn(8, 25 * (n + 2 * K) + 148, generator=g).to(dev)
        eng = build(8, n // S, solver=solver)
        known = torch.randn(8, 2 * K * 2, 32, 32, generator=g).to(dev)
        mask = A.sampler.canvas_frame_mask(known.shape, 0, known.shape[1] // 3)
        init = dict(init_canvas=known, mask=mask, guide_seed=3)
        kinds = [("unguided", {}), ("tail pass", dict(init, guided_shift=False)), ("guided shift", dict(init, guided_shift=True))]
        outs = [A.fifo_denoise(eng, canvas_p, 25, sched, 4, 5, **kw) for _, kw in kinds]      # warm-up
        assert torch.equal(outs[1], outs[2])
        ts_ = {(name, K_): [] for name, _ in kinds for K_ in (K, 2 * K)}
        for _ in range(args.rounds):
            for K_ in (K, 2 * K):
                for name, kw in kinds:
                    ts_[name, K_].append(timed(lambda: A.fifo_denoise(eng, canvas_p, 25, sched, K_, 5, **kw)))
        per = {}
        for name, _ in kinds:
            whole = {K_: statistics.median(ts_[name, K_]) for K_ in (K, 2 * K)}
            per[name] = (whole[2 * K] - whole[K]) / K
            print(f"  {solver:8s} n = {n}, B = {n // S}, {name:12s}: " +
                  "; ".join(f"{K_} out " + " ".join(f"{t * 1e3:7.1f}" for t in ts_[name, K_]) for K_ in (K, 2 * K)) +
                  f"; per finished slot {per[name] * 1e3:.3f}, ramp and start {(whole[K] - K * per[name]) * 1e3:.1f}")
        print(f"  {'':8s} per finished slot, guided shift against tail pass: {(per['guided shift'] - per['tail pass']) * 1e6:+.1f} us "
              f"(x {per['guided shift'] / per['tail pass']:.4f})")
    sys.exit(0)

if args.guide and args.kernels:
    B, S, sl = 32, 6, 2
    g = torch.Generator().manual_seed(0)
    z = torch.randn(B, 8, 12, 32, 32, generator=g).to(dev)
    prompt = torch.randn(B, 8, 150, generator=g).to(dev)
    out = torch.empty_like(z)
    known = torch.randn(8, B * 12, 32, 32, generator=g).to(dev)      # the clip under the whole batch: two more 25 MB streams
    mask = torch.rand(8, B * 12, 32, 32, generator=g).to(dev)
    PLAIN, GUIDED = "cfg_unpatch_ddim_kernel", "cfg_unpatch_ddim_kernel<clip guide>"
    rows = []
    for solver, eta, n in (("ddim", 0.0, 48), ("ddim", 0.5, 48), ("dpmpp_2m", 0.0, 18), ("dpmpp_2m", 1.0, 18)):
        dpm = solver == "dpmpp_2m"
        sched = su.make_sampling_schedule(1000, n)
        eng = build(2, B, solver=solver, eta=eta, **({"noise_seed": 11} if eta else {}))
        eng.set_prompt(prompt)
        if dpm:
            eng.x0_hist.copy_(torch.randn(B, 8, 12, 32, 32, generator=g))
        i = (torch.arange(B * S) % (n - 2)).view(B, S) + 1      # the diagonal: none held, none final
        tlS, tnS, tpS = (sched[i + d].to(dev).contiguous() for d in (-1, 0, 1))
        last = dict(t_last=tlS) if dpm else {}

        def step(guided, eng=eng, last=last, tnS=tnS, tpS=tpS):
            if guided:      # "mask": a fractional mask canvas, one more stream than "no mask" (1 everywhere)
                eng.set_clip_guide(known, mask if guided == "mask" else None, guide_seed=3)
            else:
                eng.clear_clip_guide()
            return lambda: eng.step_slots(z, tnS, tpS, out=out, clip_first=0, **last)

        name = f"{solver} eta = {eta}"
        rows += [(f"{name}, unguided (a)", PLAIN, step, False), (f"{name}, clip guide", GUIDED, step, "mask"),
                 (f"{name}, clip guide, no mask", GUIDED, step, "no mask"), (f"{name}, unguided (b)", PLAIN, step, False)]
    zq = torch.randn(8, 8, 12, 32, 32, generator=g).to(dev)          # the e2e queue at n = 48: B = 8
    every = {b: torch.full((b, S), 999, dtype=torch.long, device=dev) for b in (B, 8)}
    tail = {b: torch.full((b, S), Fn.SLOT_LEAVE, dtype=torch.long, device=dev) for b in (B, 8)}
    for b in (B, 8):
        tail[b][b - 1, S - 1] = 999
    kw = dict(slot_len=sl, seed=3)
    PASS = "clip_guide_slots_kernel<4>"
    for zz in (z, zq):
        b = zz.shape[0]
        rows += [(f"fifo_shift B={b}", "fifo_shift_kernel<4>", lambda g_, zz=zz, b=b: (lambda: Fn.fifo_shift(zz, b * S, 7, 999, sl)), None),
                 (f"guide pass, all slots B={b}", PASS, lambda g_, zz=zz, b=b: (lambda: Fn.clip_guide_slots(known, every[b], ABAR_D, zz, mask,
                                                                                                          out=out[:b], **kw)), None),
                 (f"guide pass, tail slot in place B={b}", PASS, lambda g_, zz=zz, b=b: (lambda: Fn.clip_guide_slots(
                     known, tail[b], ABAR_D, zz, mask, first=1, out=zz, **kw)), None)]
    ABAR_D = ABAR.to(dev)
    for _, _, mk, guided in rows:
        fn = mk(guided)
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    res = {name: [] for name, _, _, _ in rows}
    for _ in range(args.rounds):
        for name, tag, mk, guided in rows:
            res[name].append(per_launch_us(tag, mk(guided), args.launches))
    print(f"C3 geometry, B = {B}: the fused CFG + un-patch + solver slot update inside whole steps (2 layers), unguided (tag {PLAIN}) and "
          f"under a clip-keyed latent guide with a fractional mask (tag {GUIDED}); the stand-alone guide pass beside the queue shift: "
          f"{args.rounds} interleaved rounds of {args.launches} launches, microseconds per launch (launch events)")
    for name, _, _, _ in rows:
        v = res[name]
        print(f"  {name:40s} " + " ".join(f"{x:8.2f}" for x in v) + f"   median {statistics.median(v):8.2f}")
    sys.exit(0)

if args.guide and args.e2e:
    S, K = 6, args.slots_out
    g = torch.Generator().manual_seed(1)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    print(f"fifo_denoise unguided and with init_canvas (clip-keyed latent guide, frames kept on a third of the clip), S = {S} (C3 latent, "
          f"8 layers, bf16x3, eager), {args.rounds} rounds, the calls interleaved, {K} and {2 * K} slots out; milliseconds")
    for solver, eta, n in (("ddim", 0.0, 48), ("dpmpp_2m", 0.0, 18)):
        sched = su.make_sampling_schedule(1000, n)
        canvas_p = torch.randn(8, 25 * (n + 2 * K) + 148, generator=g).to(dev)
        eng = build(8, n // S, solver=solver)
        known = torch.randn(8, 2 * K * 2, 32, 32, generator=g).to(dev)
        mask = A.sampler.canvas_frame_mask(known.shape, 0, known.shape[1] // 3)
        kinds = [("unguided", {}), ("init_canvas", dict(init_canvas=known, mask=mask, guide_seed=3))]
        for _, kw in kinds:
            A.fifo_denoise(eng, canvas_p, 25, sched, 4, 5, **kw)      # warm-up
        ts_ = {(name, K_): [] for name, _ in kinds for K_ in (K, 2 * K)}
        for _ in range(args.rounds):
            for K_ in (K, 2 * K):
                for name, kw in kinds:
                    ts_[name, K_].append(timed(lambda: A.fifo_denoise(eng, canvas_p, 25, sched, K_, 5, **kw)))
        per = {}
        for name, _ in kinds:
            whole = {K_: statistics.median(ts_[name, K_]) for K_ in (K, 2 * K)}
            per[name] = (whole[2 * K] - whole[K]) / K
            print(f"  {solver:8s} n = {n}, B = {n // S}, {name:11s}: " +
                  "; ".join(f"{K_} out " + " ".join(f"{t * 1e3:7.1f}" for t in ts_[name, K_]) for K_ in (K, 2 * K)) +
                  f"; per finished slot {per[name] * 1e3:.3f}, ramp and start {(whole[K] - K * per[name]) * 1e3:.1f}")
        a, b = (per[name] for name, _ in kinds)
        print(f"  {'':8s} per finished slot, guided against unguided: {(b - a) * 1e3:+.3f} ms (x {b / a:.3f})")
    sys.exit(0)

if args.stochastic and args.kernels:
    B, S = 32, 6
    g = torch.Generator().manual_seed(0)
    z = torch.randn(B, 8, 12, 32, 32, generator=g).to(dev)
    prompt = torch.randn(B, 8, 150, generator=g).to(dev)
    out = torch.empty_like(z)
    TAG = "cfg_unpatch_ddim_kernel"
    rows = []
    for solver, eta, n in STOCHASTIC:
        dpm = solver == "dpmpp_2m"
        sched = su.make_sampling_schedule(1000, n)
        det = build(2, B, solver=solver)
        sto = build(2, B, solver=solver, eta=eta, noise_seed=11)
        can = build(2, B, solver=solver, eta=eta, noise_seed=11, noise_keying="canvas", canvas_hop=12)
        for e in (det, sto, can):
            e.set_prompt(prompt)
            if dpm:
                e.x0_hist.copy_(torch.randn(B, 8, 12, 32, 32, generator=g))
        # the diagonal: every slot at its own level (second-order triples for dpmpp_2m), none held, none final
        i = (torch.arange(B * S) % (n - 2)).view(B, S) + 1
        tlS, tnS, tpS = (sched[i + d].to(dev).contiguous() for d in (-1, 0, 1))
        tl1, tn1, tp1 = (torch.full((B,), int(sched[5 + d]), dtype=torch.long, device=dev) for d in (-1, 0, 1))
        last = dict(t_last=tlS) if dpm else {}
        last1 = dict(t_last=tl1) if dpm else {}
        rows += [(f"{solver} slots, eta = 0 (a)", lambda det=det, last=last, tnS=tnS, tpS=tpS: det.step_slots(z, tnS, tpS, out=out, **last)),
                 (f"{solver} slots, eta = {eta}, clip-keyed", lambda sto=sto, last=last, tnS=tnS, tpS=tpS:
                  sto.step_slots(z, tnS, tpS, out=out, clip_first=0, **last)),
                 (f"{solver} slots, eta = 0 (b)", lambda det=det, last=last, tnS=tnS, tpS=tpS: det.step_slots(z, tnS, tpS, out=out, **last)),
                 (f"{solver} per-sample, eta = {eta}, canvas-keyed", lambda can=can, last1=last1, tn1=tn1, tp1=tp1:
                  can.step(z, tn1, tp1, out=out, **last1)),
                 (f"{solver} per-sample, eta = 0", lambda det=det, last1=last1, tn1=tn1, tp1=tp1: det.step(z, tn1, tp1, out=out, **last1))]
    for _, fn in rows:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    res = {name: [] for name, _ in rows}
    for _ in range(args.rounds):
        for name, fn in rows:
            res[name].append(per_launch_us(TAG, fn, args.launches))
    print(f"C3 geometry, B = {B}, the fused CFG + un-patch + solver update inside whole steps (2 layers), tag {TAG}: {args.rounds} interleaved "
          f"rounds of {args.launches} launches, microseconds per launch (launch events)")
    for name, _ in rows:
        v = res[name]
        print(f"  {name:46s} " + " ".join(f"{x:8.2f}" for x in v) + f"   median {statistics.median(v):8.2f}")
    sys.exit(0)

if args.stochastic and args.e2e:
    S, K = 6, args.slots_out
    g = torch.Generator().manual_seed(1)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    print(f"fifo_denoise at eta = 0 and at eta > 0 (clip-keyed slot noise), S = {S} (C3 latent, 8 layers, bf16x3), {args.rounds} rounds, the two "
          f"engines' calls interleaved, {K} and {2 * K} slots out; milliseconds")
    for solver, eta, n in STOCHASTIC:
        sched = su.make_sampling_schedule(1000, n)
        canvas_p = torch.randn(8, 25 * (n + 2 * K) + 148, generator=g).to(dev)
        engines = [("eta = 0", build(8, n // S, solver=solver)), (f"eta = {eta}", build(8, n // S, solver=solver, eta=eta, noise_seed=11))]
        for graph in (False, True):
            for _, eng in engines:
                A.fifo_denoise(eng, canvas_p, 25, sched, 4, 5, graph=graph)      # warm-up
            ts_ = {(name, K_): [] for name, _ in engines for K_ in (K, 2 * K)}
            for _ in range(args.rounds):
                for K_ in (K, 2 * K):
                    for name, eng in engines:
                        ts_[name, K_].append(timed(lambda: A.fifo_denoise(eng, canvas_p, 25, sched, K_, 5, graph=graph)))
            per = {}
            for name, eng in engines:
                whole = {K_: statistics.median(ts_[name, K_]) for K_ in (K, 2 * K)}
                per[name] = (whole[2 * K] - whole[K]) / K
                print(f"  {solver:8s} n = {n}, B = {n // S}, {'replayed' if graph else 'eager':8s} {name:9s}: " +
                      "; ".join(f"{K_} out " + " ".join(f"{t * 1e3:7.1f}" for t in ts_[name, K_]) for K_ in (K, 2 * K)) +
                      f"; per finished slot {per[name] * 1e3:.3f}, ramp and start {(whole[K] - K * per[name]) * 1e3:.1f}")
            a, b = (per[name] for name, _ in engines)
            print(f"  {'':8s} per finished slot, eta > 0 against eta = 0: {(b - a) * 1e3:+.3f} ms (x {b / a:.3f})")
    sys.exit(0)

if args.kernels and args.lookahead:
    S, ctx, sl = 6, args.lookahead, 2
    h = S - ctx
    g = torch.Generator().manual_seed(0)
    # B = 32 as the other kernel records; then the queues of --e2e --lookahead at n = 48 and n = 18 when h divides them
    sizes = [32] + [n // h for n in (48, 18) if n % h == 0]
    rows, meta = [], {}
    for B in sizes:
        z, hz = torch.randn(B, 8, 12, 32, 32, generator=g).to(dev), torch.randn(B, 8, 12, 32, 32, generator=g).to(dev)
        slot = z[0, :, :sl].numel()
        Q = ctx + B * h

        def add(name, tag, fn, nbytes):
            rows.append((name, tag, fn))
            meta[name] = nbytes

        add(f"fifo_shift B={B}", "fifo_shift_kernel<4>", lambda z=z, B=B: Fn.fifo_shift(z, B * S, 7, 999, sl), 4 * (2 * z.numel() + slot))
        add(f"fifo_shift+hist B={B}", "fifo_shift_kernel<4, HistShift>", lambda z=z, hz=hz, B=B: Fn.fifo_shift(z, B * S, 7, 999, sl, hist=hz),
            4 * (4 * z.numel() + slot))
        for shift in (0, 1):
            kw = dict(c=B * h, seed=7, t=999) if shift else {}
            # every owner read once (Q slots; the tail is drawn, not read), B * S slots written, the popped slot written at shift 1
            nb = 4 * ((Q - shift + B * S) * slot + shift * slot)
            add(f"lookahead shift={shift} B={B}", "fifo_lookahead_kernel<4>",
                lambda z=z, shift=shift, kw=kw: Fn.fifo_lookahead(z, ctx, shift, sl, **kw), nb)
            # the history: owners of the active slots read, B * h stepping slots and B * ctx zero slots written
            nbh = nb + 4 * ((B * h - shift) + B * S) * slot
            add(f"lookahead+hist shift={shift} B={B}", "fifo_lookahead_kernel<4, hist>",
                lambda z=z, hz=hz, shift=shift, kw=kw: Fn.fifo_lookahead(z, ctx, shift, sl, hist=hz, **kw), nbh)
    for _, _, fn in rows:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    res = {name: [] for name, _, _ in rows}
    for _ in range(args.rounds):
        for name, tag, fn in rows:
            res[name].append(per_launch_us(tag, fn, args.launches))
    print(f"C3 geometry (latent [B, 8, 12, 32, 32], S = {S} slots of {sl} latent frames), lookahead ctx = {ctx} (h = {h}): the lookahead "
          f"launch beside the plain shift, {args.rounds} interleaved rounds of {args.launches} launches, microseconds per launch (launch events)")
    for name, _, _ in rows:
        v = res[name]
        us = statistics.median(v)
        print(f"  {name:32s} " + " ".join(f"{x:8.2f}" for x in v) + f"   median {us:8.2f}   {meta[name] / 1e6:7.2f} MB, "
              f"{meta[name] / us:8.0f} bytes per microsecond")
    sys.exit(0)

if args.kernels and DPM:
    B, S = 32, 6
    eng = build(2, B, solver="dpmpp_2m")
    g = torch.Generator().manual_seed(0)
    z = torch.randn(B, 8, 12, 32, 32, generator=g).to(dev)
    eng.set_prompt(torch.randn(B, 8, 150, generator=g).to(dev))
    eng.x0_hist.copy_(torch.randn(B, 8, 12, 32, 32, generator=g))
    out = torch.empty_like(z)
    sched = su.make_sampling_schedule(1000, 18)
    tl1, tn1, tp1 = (torch.full((B,), int(v), dtype=torch.long, device=dev) for v in (sched[5], sched[6], sched[7]))      # second order
    i = (torch.arange(B * S) % 16).view(B, S) + 1                              # the diagonal: second-order triples, one per slot
    tlS, tnS, tpS = (sched[i + d].to(dev).contiguous() for d in (-1, 0, 1))
    tnH, tpH = tnS.clone(), tpS.clone()
    tpH[:, S // 2:] = tnH[:, S // 2:]                                          # half of every sample held
    zq = torch.randn(3, 8, 12, 32, 32, generator=g).to(dev)                    # the e2e queue at n = 18: B = 3
    hq = torch.randn(3, 8, 12, 32, 32, generator=g).to(dev)
    hz = eng.x0_hist.clone()
    TAG = "cfg_unpatch_ddim_kernel"
    rows = [("DPM update per-sample (a)", TAG, lambda: eng.step(z, tn1, tp1, out=out, t_last=tl1)),
            ("DPM update slots, diagonal", TAG, lambda: eng.step_slots(z, tnS, tpS, out=out, t_last=tlS)),
            ("DPM update per-sample (b)", TAG, lambda: eng.step(z, tn1, tp1, out=out, t_last=tl1)),
            ("DPM update slots, half held", TAG, lambda: eng.step_slots(z, tnH, tpH, out=out, t_last=tlS)),
            ("fifo_shift B=32", "fifo_shift_kernel<4>", lambda: Fn.fifo_shift(z, 192, 7, 999, 2)),
            ("fifo_shift+hist B=32", "fifo_shift_kernel<4, HistShift>", lambda: Fn.fifo_shift(z, 192, 7, 999, 2, hist=hz)),
            ("fifo_shift B=3", "fifo_shift_kernel<4>", lambda: Fn.fifo_shift(zq, 18, 7, 999, 2)),
            ("fifo_shift+hist B=3", "fifo_shift_kernel<4, HistShift>", lambda: Fn.fifo_shift(zq, 18, 7, 999, 2, hist=hq))]
    for _, _, fn in rows:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    res = {name: [] for name, _, _ in rows}
    for _ in range(args.rounds):
        for name, tag, fn in rows:
            res[name].append(per_launch_us(tag, fn, args.launches))
    print(f"C3 geometry, B = {B}, the fused CFG + un-patch + DPM-Solver++(2M) update inside whole steps (2 layers) and the queue shifts: "
          f"{args.rounds} interleaved rounds of {args.launches} launches, microseconds per launch (launch events)")
    for name, _, _ in rows:
        v = res[name]
        print(f"  {name:28s} " + " ".join(f"{x:8.2f}" for x in v) + f"   median {statistics.median(v):8.2f}")
    report_shift(res, (("fifo_shift B=32", z, 2), ("fifo_shift+hist B=32", z, 4), ("fifo_shift B=3", zq, 2), ("fifo_shift+hist B=3", zq, 4)))

if args.kernels and not DPM:
    B, S = 32, 6
    eng = build(2, B)
    g = torch.Generator().manual_seed(0)
    z = torch.randn(B, 8, 12, 32, 32, generator=g).to(dev)
    eng.set_prompt(torch.randn(B, 8, 150, generator=g).to(dev))
    eps2 = torch.randn(2 * B, 384, 256, generator=g).to(dev)
    out = torch.empty_like(z)
    ab, st, lib = ABAR.to(dev), L.stream_ptr(dev), L.lib()
    sched = su.make_sampling_schedule(1000, 48)
    tn1, tp1 = (torch.full((B,), int(v), dtype=torch.long, device=dev) for v in (sched[10], sched[11]))
    # the diagonal of a FIFO queue: every slot of the batch at its own level (6 consecutive pairs per sample, repeated over the batch)
    i = (torch.arange(B * S) % 47).view(B, S)
    tnS, tpS = sched[i].to(dev).contiguous(), sched[i + 1].to(dev).contiguous()
    tnH, tpH = tnS.clone(), tpS.clone()
    tpH[:, S // 2:] = tnH[:, S // 2:]                     # half of every sample held
    head = (eps2.data_ptr(), z.data_ptr())
    dims = (B, 8, 12, 32, 32, 2, 4, 4, st)

    def update(tn, tp, slots):
        if slots:
            return lambda: L.check(lib.avd_cfg_unpatch_ddim_slots_f32(*head, tn.data_ptr(), tp.data_ptr(), ab.data_ptr(), 1000, 3.5, slots,
                                                                      out.data_ptr(), *dims))
        return lambda: L.check(lib.avd_cfg_unpatch_ddim_f32(*head, tn.data_ptr(), tp.data_ptr(), ab.data_ptr(), 1000, 3.5, 0.0, None,
                                                            out.data_ptr(), *dims))

    e = eng.embed
    tok = torch.empty(lib.avd_embed_workspace_floats(C.byref(e)), device=dev)
    X2 = torch.empty(2 * B, eng.N, eng.d, device=dev)
    emb = (C.byref(e), z.data_ptr(), eng._aw.data_ptr(), eng._ab.data_ptr())

    def embed(tn, slots):
        if slots:
            return lambda: L.check(lib.avd_embed_cfg_pair_slots_f32(*emb, tn.data_ptr(), slots, eng.Xp.data_ptr(), tok.data_ptr(),
                                                                    X2.data_ptr(), st))
        return lambda: L.check(lib.avd_embed_cfg_pair_f32(*emb, tn.data_ptr(), eng.Xp.data_ptr(), tok.data_ptr(), X2.data_ptr(), st))

    zq = torch.randn(8, 8, 12, 32, 32, generator=g).to(dev)          # the e2e queue: B = 8
    rows = [("update per-sample (a)", "cfg_unpatch_ddim_kernel", update(tn1, tp1, 0)),
            ("update slots, diagonal", "cfg_unpatch_ddim_kernel", update(tnS, tpS, S)),
            ("update per-sample (b)", "cfg_unpatch_ddim_kernel", update(tn1, tp1, 0)),
            ("update slots, half held", "cfg_unpatch_ddim_kernel", update(tnH, tpH, S)),
            ("assembly per-sample (a)", "assemble_rows_kernel", embed(tn1, 0)),
            ("assembly slots", "assemble_rows_kernel", embed(tnS, S)),
            ("assembly per-sample (b)", "assemble_rows_kernel", embed(tn1, 0)),
            ("fifo_shift B=32", "fifo_shift_kernel<4>", lambda: Fn.fifo_shift(z, 192, 7, 999, 2)),
            ("fifo_shift B=8", "fifo_shift_kernel<4>", lambda: Fn.fifo_shift(zq, 48, 7, 999, 2))]
    for _, _, fn in rows:
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    res = {name: [] for name, _, _ in rows}
    for _ in range(args.rounds):
        for name, tag, fn in rows:
            res[name].append(per_launch_us(tag, fn, args.launches))
    print(f"C3 geometry, {args.rounds} interleaved rounds of {args.launches} launches, microseconds per launch (launch events)")
    for name, _, _ in rows:
        v = res[name]
        print(f"  {name:28s} " + " ".join(f"{x:8.2f}" for x in v) + f"   median {statistics.median(v):8.2f}")
    report_shift(res, (("fifo_shift B=32", z, 2), ("fifo_shift B=8", zq, 2)))

if args.e2e and args.lookahead:
    S, K, ctx = 6, args.slots_out, args.lookahead
    h = S - ctx
    n = args.steps or (18 if DPM else 48)
    if n % S or n % h:
        raise SystemExit(f"--steps {n} must be a multiple of S = {S} and of h = S - ctx = {h}")
    sched = su.make_sampling_schedule(1000, n)
    g = torch.Generator().manual_seed(1)
    canvas_p = torch.randn(8, 25 * (n + 2 * K) + 148, generator=g).to(dev)
    hop_p = 25

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    print(f"fifo_denoise with and without lookahead: solver {args.solver}, n = {n} steps, S = {S} (C3 latent, 8 layers, bf16x3, eager), "
          f"{args.rounds} rounds, the two queues' calls interleaved")
    queues = [("plain queue", 0, build(8, n // S, solver=args.solver)), (f"lookahead ctx = {ctx}", ctx, build(8, n // h, solver=args.solver))]
    for _, la, eng in queues:
        A.fifo_denoise(eng, canvas_p, hop_p, sched, 4, 5, lookahead=la)      # warm-up
    ts_ = {(name, K_): [] for name, _, _ in queues for K_ in (K, 2 * K)}
    for _ in range(args.rounds):
        for K_ in (K, 2 * K):
            for name, la, eng in queues:
                ts_[name, K_].append(timed(lambda: A.fifo_denoise(eng, canvas_p, hop_p, sched, K_, 5, lookahead=la)))
    per = {}
    for name, la, eng in queues:
        whole = {K_: statistics.median(ts_[name, K_]) for K_ in (K, 2 * K)}
        per[name] = (whole[2 * K] - whole[K]) / K
        print(f"  {name:20s} B = {eng.embed.B:2d}: " + "; ".join(f"{K_} slots out " + " ".join(f"{t * 1e3:7.1f}" for t in ts_[name, K_]) + " ms"
                                                                   for K_ in (K, 2 * K)))
        print(f"  {'':20s} per finished slot (steady state, from the two clip lengths) {per[name] * 1e3:.3f} ms; ramp of {n - 1} steps and "
              f"start {(whole[K] - K * per[name]) * 1e3:.1f} ms")
    a, b = (per[name] for name, _, _ in queues)
    print(f"  per finished slot, lookahead / plain: x {b / a:.2f} (at most S / h = {S / h:.2f}: one step at B = {n // h} against one at B = {n // S})")
    sys.exit(0)

if args.e2e:
    S, K = 6, args.slots_out
    n = args.steps or (18 if DPM else 48)
    if n % S:
        raise SystemExit(f"--steps {n} must be a multiple of S = {S}")
    B = n // S
    sched = su.make_sampling_schedule(1000, n)
    eng = build(8, B, solver=args.solver)
    g = torch.Generator().manual_seed(1)
    canvas_p = torch.randn(8, 25 * (n + 2 * K) + 148, generator=g).to(dev)      # 25 audio latent frames per target slot of 2 latent frames
    hop_p = 25

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    A.fifo_denoise(eng, canvas_p, hop_p, sched, 4, 5, graph=args.graph)      # warm-up
    print(f"fifo_denoise: solver {args.solver}, n = {n} steps, S = {S}, B = {B} (C3 latent, 8 layers, bf16x3, "
          f"{'graph replay' if args.graph else 'eager'}), {args.rounds} rounds")
    whole = {}
    for K_ in (K, 2 * K):
        ts_ = [timed(lambda: A.fifo_denoise(eng, canvas_p, hop_p, sched, K_, 5, graph=args.graph))[0] for _ in range(args.rounds)]
        whole[K_] = statistics.median(ts_)
        print(f"  {K_:3d} slots out: " + " ".join(f"{t * 1e3:8.1f}" for t in ts_) + f" ms   ({K_ / statistics.median(ts_):6.1f} slots/s whole call, "
              f"ramp of {n - 1} steps included)")
    # two clip lengths separate the two costs: the difference is K steady iterations, the rest of the shorter call is the ramp
    per_slot = (whole[2 * K] - whole[K]) / K
    print(f"  per finished slot (steady state, from the two clip lengths): {per_slot * 1e3:.3f} ms; ramp of {n - 1} steps: "
          f"{(whole[K] - K * per_slot) * 1e3:.1f} ms")
    if args.graph:
        # what the call pays for its two graphs: each capture on an open queue whose phase has run once (no replay: the cursors stay)
        caps = {"ramp pair": [], "steady pair": []}
        for _ in range(args.rounds):
            q = eng.fifo_open(canvas_p, hop_p, fifo_prompt_len(eng, canvas_p), sched, K, 5)
            eng.fifo_ramp(q, q.z, q.other)
            eng.fifo_steady(q, q.other, q.z)
            caps["ramp pair"].append(timed(lambda: eng.fifo_capture(q, False, q.other, q.z))[0])
            caps["steady pair"].append(timed(lambda: eng.fifo_capture(q, True, q.other, q.z))[0])
        print("  capture (torch.cuda.graph around two iterations, synchronise included): " +
              "; ".join(f"{k} " + " ".join(f"{t * 1e3:6.2f}" for t in v) + " ms" for k, v in caps.items()))
        sys.exit(0)
    # the parts of a steady iteration, each ended by a synchronise
    rn, rp, sn, sp = (t.to(dev) for t in su.fifo_plan(sched, S))
    sl = su.fifo_plan_last(sched, S)[1].to(dev) if DPM else None
    Lp = fifo_prompt_len(eng, canvas_p)
    z = Fn.canvas_noise(5, torch.full((B,), int(sched[0])), eng.latent_shape, 12)
    parts = {"set_prompt": [], "step_slots": [], "fifo_shift": []}
    for m in range(3 * args.rounds * 4):
        t, _ = timed(lambda: eng.set_prompt(fifo_prompt_windows(canvas_p, m, B, S, hop_p, Lp)))
        parts["set_prompt"].append(t)
        t, zo = timed(lambda: eng.step_slots(z, sn, sp, t_last=sl))
        parts["step_slots"].append(t)
        t, (z, _) = timed(lambda: eng.fifo_shift(zo, n + m, int(sched[0]), seed=5))
        parts["fifo_shift"].append(t)
    med = {k: statistics.median(v[4:]) for k, v in parts.items()}
    tot = sum(med.values())
    print("  steady iteration (one finished slot), parts timed with a synchronise after each: " +
          ", ".join(f"{k} {v * 1e3:.3f} ms ({100 * v / tot:.1f} %)" for k, v in med.items()) + f"; {1 / tot:.1f} slots/s steady state")
    if DPM:
        sys.exit(0)
    # the window-consensus loop at the same step count: 8 windows of 12 latent frames, hop 4 (the 3 s / 1 s default): a canvas of 40
    # latent frames = 20 slots of 2 frames
    engc = build(8, B)
    engc.set_prompt(torch.randn(B, 8, 150, generator=g).to(dev))
    engc.set_window_consensus(4)
    z0 = torch.randn(B, 8, 12, 32, 32, generator=g).to(dev)
    engc.run(z0, sched[:4])
    ts_ = [timed(lambda: engc.run(z0, sched))[0] for _ in range(args.rounds)]
    print(f"window consensus (DenoiseEngine.run, set_window_consensus(4), B = {B} windows of 12 frames: 20 slots of 2 frames), {n} steps: " +
          " ".join(f"{t * 1e3:8.1f}" for t in ts_) + f" ms   ({20 / statistics.median(ts_):6.1f} slots/s)")
