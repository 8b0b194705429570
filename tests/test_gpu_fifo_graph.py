"""FIFO diagonal denoising replayed from HIP graphs: the three kernels that read a device cursor (prompt gather, queue shift, slot-table
select) against the host forms they replace, and ``fifo_denoise(graph=True)`` against the eager call — everything bit for bit, the
feature adds no arithmetic."""
import ctypes as C

import pytest
import torch

import _slot_ref as SR
from _kit import dev, engine, model  # noqa: F401  (dev, model are fixtures)

pytestmark = pytest.mark.gpu

GS = 3.5
SEED = 0x5EED0F1F0
SCHED4 = torch.tensor([999, 749, 499, 249, -1])
SCHED6 = torch.tensor([999, 832, 666, 499, 332, 166, -1])
SHIFT_SHAPES = [((2, 8, 4, 16, 16), 2), ((2, 8, 40), 4), ((3, 8, 4, 16, 16), 1)]


def cur(dev, v):
    return torch.tensor([v], dtype=torch.int32, device=dev)


def off(x):
    """a copy of x whose base is misaligned by one float"""
    v = torch.empty(x.numel() + 1, device=x.device)[1:].view(x.shape).copy_(x)
    assert v.data_ptr() % 16 != 0
    return v


# ------------------------------------------------------------------------------------------------- 1. prompt gather
def _situation(P, m, B, S, hop, ln):
    """where the B samples of steady iteration m lie on a canvas of P positions"""
    starts = [(m + k * S) * hop for k in range(B)]
    if all(p0 + ln <= P for p0 in starts):
        return "inside"
    return "zeros" if all(p0 >= P for p0 in starts) else "partly"


@pytest.mark.parametrize("kind", ["audio", "video"])
def test_prompt_gather_equals_fifo_prompt_windows(dev, kind):
    from multimodal_diffusion_amd import functional as Fn
    from multimodal_diffusion_amd.stream_infer import fifo_prompt_windows
    g = torch.Generator().manual_seed(3)
    B, S = 2, 2
    if kind == "audio":
        canvas, hop, ln = torch.randn(8, 150, generator=g).to(dev), 20, 40          # inner = 1: one element per lane
        ms = (0, 3, 5, 8)
    else:
        canvas, hop, ln = torch.randn(8, 14, 8, 8, generator=g).to(dev), 2, 4       # inner = 64: 16-byte lanes
        assert canvas.data_ptr() % 16 == 0
        by = {}
        for m in range(0, 14):
            by.setdefault(_situation(14, m, B, S, hop, ln), []).append(m)
        ms = (by["inside"][0], by["inside"][-1], by["partly"][len(by["partly"]) // 2], by["zeros"][0])
    P = canvas.shape[1]
    assert [_situation(P, m, B, S, hop, ln) for m in ms] == ["inside", "inside", "partly", "zeros"] and ms[0] == 0 and ms[1] > 0
    mis = off(canvas)
    for m in ms:
        ref = fifo_prompt_windows(canvas, m, B, S, hop, ln)
        out = Fn.fifo_prompt_gather(canvas, cur(dev, m), B, S, hop, ln)
        assert out.shape == ref.shape and torch.equal(out, ref), m
        if _situation(P, m, B, S, hop, ln) == "zeros":
            assert not out.any()
        # a misaligned canvas, and a misaligned out, take the one-element lanes: same bits
        assert torch.equal(Fn.fifo_prompt_gather(mis, cur(dev, m), B, S, hop, ln), ref), m
        o2 = off(torch.full_like(ref, float("nan")))
        assert torch.equal(Fn.fifo_prompt_gather(canvas, cur(dev, m), B, S, hop, ln, out=o2), ref), m
    # a negative cursor is clamped to 0; one far past the canvas reads nothing
    ref0 = fifo_prompt_windows(canvas, 0, B, S, hop, ln)
    for m in (-1, -2 ** 31):
        assert torch.equal(Fn.fifo_prompt_gather(canvas, cur(dev, m), B, S, hop, ln), ref0), m
    assert not Fn.fifo_prompt_gather(canvas, cur(dev, 2 ** 31 - 1), B, S, hop, ln).any()
    # an out that overlaps the canvas is refused
    n_out = ref0.numel()
    both = torch.zeros(canvas.numel() + n_out - 4, device=dev)
    c2, o2 = both[:canvas.numel()].view(canvas.shape), both[canvas.numel() - 4:].view(ref0.shape)
    with pytest.raises(ValueError, match="overlap"):
        Fn.fifo_prompt_gather(c2, cur(dev, 0), B, S, hop, ln, out=o2)


# ------------------------------------------------------------------------------------------------- 2. cursor shift
@pytest.mark.parametrize("with_hist", [False, True])
@pytest.mark.parametrize("shape,slot_len", SHIFT_SHAPES)
def test_cursor_shift_equals_the_by_value_shift(dev, shape, slot_len, with_hist):
    from multimodal_diffusion_amd import functional as Fn
    g = torch.Generator().manual_seed(len(shape) + slot_len)
    z, hist = torch.randn(shape, generator=g).to(dev), torch.randn(shape, generator=g).to(dev)
    c0, t, n_out, sentinel = 11, 999, 4, -7.0
    clip_shape = (shape[1], n_out * slot_len) + tuple(shape[3:])

    def run(m, zi=z, hi=hist, clip=None, ho=None):
        clip = torch.full(clip_shape, sentinel, device=dev) if clip is None else clip
        r = Fn.fifo_shift_cursor(zi, c0, cur(dev, m), clip, SEED, t, slot_len, hist=hi if with_hist else None,
                                 hist_out=ho if with_hist else None)
        return (r if with_hist else (r, None)) + (clip,)

    def expected(m, popped):
        want = torch.full(clip_shape, sentinel, device=dev)
        if 0 <= m < n_out:
            want[:, m * slot_len:(m + 1) * slot_len] = popped                    # slot m is the popped head, nothing else is touched
        return want

    for m in (0, 2, n_out - 1, n_out, -1):
        ref = Fn.fifo_shift(z, c0 + m, SEED, t, slot_len, hist=hist if with_hist else None)
        out, hist_out, clip = run(m)
        assert torch.equal(out, ref[0]), m
        if with_hist:
            assert torch.equal(hist_out, ref[2]), m
        assert torch.equal(clip, expected(m, ref[1])), m
        # misaligned bases take the one-element lanes: same bits
        for which in ("z", "clip") + (("hist", "hist_out") if with_hist else ()):
            o2, h2, c2 = run(m, zi=off(z) if which == "z" else z, hi=off(hist) if which == "hist" else hist,
                             clip=off(torch.full(clip_shape, sentinel, device=dev)) if which == "clip" else None,
                             ho=off(hist) if which == "hist_out" else None)
            assert torch.equal(o2, out) and torch.equal(c2, expected(m, ref[1])), (m, which)
            if with_hist:
                assert torch.equal(h2, hist_out), (m, which)


def test_cursor_shift_refusals(dev):
    from multimodal_diffusion_amd import _lib as L
    from multimodal_diffusion_amd import functional as Fn
    z, hist = torch.randn(2, 8, 40, device=dev), torch.randn(2, 8, 40, device=dev)
    clip = torch.zeros(8, 16, device=dev)
    m = cur(dev, 0)
    with pytest.raises(ValueError, match="overlap"):
        Fn.fifo_shift_cursor(z, 4, m, clip, SEED, 999, 4, out=z)                              # in place
    with pytest.raises(ValueError, match="overlap"):
        Fn.fifo_shift_cursor(z, 4, m, z.view(-1)[:128].view(8, 16), SEED, 999, 4)                # the clip canvas lies in the queue
    both = torch.zeros(z.numel() + 128 - 4, device=dev)                                       # the canvas shares the history's last floats
    h_in, c_in = both[:z.numel()].view_as(z), both[z.numel() - 4:].view(8, 16)
    with pytest.raises(ValueError, match="overlap"):
        Fn.fifo_shift_cursor(z, 4, m, c_in, SEED, 999, 4, hist=h_in)
    with pytest.raises(ValueError, match="overlap"):
        Fn.fifo_shift_cursor(z, 4, m, c_in, SEED, 999, 4, hist=hist, hist_out=h_in)
    with pytest.raises(ValueError, match="overlap"):
        Fn.fifo_shift_cursor(z, 4, m, clip, SEED, 999, 4, hist=hist, hist_out=hist)
    # (c0 + n_out) * slot_len > 2^32: refused by the wrapper and by the library's own check before the launch
    c0 = 2 ** 32 // 4 - 3                                                                     # (c0 + 4) * 4 = 2^32 + 4
    with pytest.raises(ValueError, match="2\\*\\*32"):
        Fn.fifo_shift_cursor(z, c0, m, clip, SEED, 999, 4)
    out = torch.empty_like(z)
    args = (m.data_ptr(), 4, z.data_ptr(), out.data_ptr(), clip.data_ptr(), 2, 8, 10, 4, 1, L.stream_ptr(dev))
    with pytest.raises(ValueError, match="2\\^32"):
        L.check(L.lib().avd_fifo_shift_cursor_f32(C.byref(Fn.noise_key(SEED, 0)), 999, c0, *args))
    L.check(L.lib().avd_fifo_shift_cursor_f32(C.byref(Fn.noise_key(SEED, 0)), 999, c0 - 1, *args))      # exactly 2^32 is allowed
    assert torch.equal(out, Fn.fifo_shift(z, c0 - 1, SEED, 999, 4)[0])
    with pytest.raises(ValueError, match="cursor"):
        Fn.fifo_shift_cursor(z, 4, torch.zeros(1, dtype=torch.long, device=dev), clip, SEED, 999, 4)


# ------------------------------------------------------------------------------------------------- 3. slot-table select
@pytest.mark.parametrize("three", [False, True])
def test_slot_tables_select_copies_the_clamped_row(dev, three):
    from multimodal_diffusion_amd import functional as Fn, schedule_utils as su
    S = 2
    rows = list(su.fifo_plan(SCHED4, S)[:2]) + ([su.fifo_plan_last(SCHED4, S)[0]] if three else [])
    n_rows, B = rows[0].shape[0], rows[0].shape[1]
    assert n_rows == 3
    tabs = [Fn.stack_slot_tables(t).to(dev) for t in rows]
    outs = [torch.full((B, S), -5, dtype=torch.long, device=dev) for _ in rows]
    for c in (0, 1, 2, 3, 7, 2 ** 31 - 1, -1, -2 ** 31):
        cursor = cur(dev, c)
        Fn.slot_tables_select(tabs, cursor, outs)
        r = min(max(c, 0), n_rows - 1)
        for o, t in zip(outs, rows):
            assert torch.equal(o.cpu(), t[r]), c                     # the row of fifo_plan / fifo_plan_last indexed on the host
        assert int(cursor) == c                                      # read, not moved
    Fn.cursor_add(cursor)
    Fn.cursor_add(cursor, 3)
    assert int(cursor) == -2 ** 31 + 4
    with pytest.raises(ValueError):
        Fn.slot_tables_select(tabs[:1], cursor, outs[:1])
    with pytest.raises(ValueError):
        Fn.slot_tables_select(tabs, cursor, [o[:1] for o in outs])


@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
def test_iteration_bodies_move_their_cursor_by_one(dev, model, solver):
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import schedule_utils as su
    from multimodal_diffusion_amd.stream_infer import fifo_prompt_len, fifo_prompt_windows
    eng, canvas_p, hop = _setup(dev, model[1], "video", solver)
    q = eng.fifo_open(canvas_p, hop, fifo_prompt_len(eng, canvas_p), SCHED4, 3, SEED)
    assert isinstance(q, A.FifoQueue) and int(q.r) == 0 and int(q.m) == 0 and len(q.ramp) == (3 if solver == "dpmpp_2m" else 2)
    xp = eng.Xp.data_ptr()
    z0 = q.z.clone()
    eng.fifo_ramp(q, q.z, q.other)
    assert int(q.r) == 1 and int(q.m) == 0
    rn, rp = su.fifo_plan(SCHED4, 2)[:2]
    assert torch.equal(q.slot[0].cpu(), rn[0]) and torch.equal(q.slot[1].cpu(), rp[0])
    rl = su.fifo_plan_last(SCHED4, 2)[0][0] if solver == "dpmpp_2m" else None
    eng.set_prompt(fifo_prompt_windows(canvas_p, 0, 2, 2, hop, 40))
    assert torch.equal(q.other, eng.step_slots(z0, rn[0], rp[0], t_last=rl))
    hist = eng.x0_hist
    eng.fifo_steady(q, q.other, q.z)
    assert int(q.r) == 1 and int(q.m) == 1 and eng.Xp.data_ptr() == xp
    if solver == "dpmpp_2m":
        assert eng.x0_hist is not hist
        eng.fifo_steady(q, q.other, q.z)
        assert eng.x0_hist is hist and int(q.m) == 2


# ------------------------------------------------------------------------------------------------- 4. the by-value shift is untouched
@pytest.mark.parametrize("shape,slot_len", SHIFT_SHAPES)
def test_by_value_shift_still_equals_roll_and_canvas_noise(dev, shape, slot_len):
    from multimodal_diffusion_amd import functional as Fn
    g = torch.Generator().manual_seed(5)
    z, hist = torch.randn(shape, generator=g).to(dev), torch.randn(shape, generator=g).to(dev)
    c, t = 13, 999
    one_slot = (1, shape[1], slot_len) + tuple(shape[3:])
    tail = Fn.canvas_noise(SEED, torch.tensor([t]), one_slot, slot_len, window_offset=c)[0]
    ref, ref_popped = SR.shift(z, tail, slot_len)
    out, popped = Fn.fifo_shift(z, c, SEED, t, slot_len)
    assert torch.equal(out, ref) and torch.equal(popped, ref_popped)
    out, popped, hist_out = Fn.fifo_shift(z, c, SEED, t, slot_len, hist=hist)
    assert torch.equal(out, ref) and torch.equal(popped, ref_popped)
    assert torch.equal(hist_out, SR.shift(hist, torch.zeros_like(tail), slot_len)[0])


# ------------------------------------------------------------------------------------------------- 5. graph == eager
def _setup(dev, mods, target, solver, B=2):
    """test_gpu_fifo._setup: a queue of B * 2 slots (S = 2), either target, either solver"""
    g = torch.Generator().manual_seed(17)
    if target == "video":
        eng = engine(mods, "video", (B, 8, 4, 16, 16), 10, guidance=GS, solver=solver)
        return eng, torch.randn(8, 150, generator=g).to(dev), 20
    eng = engine(mods, "audio", (B, 8, 8), 8, guidance=GS, solver=solver)
    return eng, torch.randn(8, 14, 8, 8, generator=g).to(dev), 2


def _both(eng, canvas_p, hop, sched, K, seed, graph=True):
    """(eager clip, replayed clip) and, on dpmpp_2m, the history each call leaves"""
    import multimodal_diffusion_amd as A
    eager = A.fifo_denoise(eng, canvas_p, hop, sched, K, seed, graph=False)
    h_e = None if eng.x0_hist is None else eng.x0_hist.clone()
    replayed = A.fifo_denoise(eng, canvas_p, hop, sched, K, seed, graph=graph)
    assert not torch.cuda.is_current_stream_capturing()
    h_g = None if eng.x0_hist is None else eng.x0_hist.clone()
    return eager, replayed, h_e, h_g


@pytest.mark.parametrize("n_slots", [1, 2, 4, 5, 8])
@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
@pytest.mark.parametrize("target", ["video", "audio"])
def test_fifo_denoise_graph_equals_eager(dev, model, target, solver, n_slots):
    """n = 4: the three ramp steps are one eager step plus one replayed pair.  n_slots 1: no steady replay; 2: eager + leftover; 4:
    eager + pair + leftover; 5: eager + two pairs; 8: eager + three pairs + leftover, and on the video target steady iterations whose
    prompt runs partly (m = 4 .. 7) and then, for the second sample, wholly (m = 6, 7) past the end of the 150-frame canvas."""
    eng, canvas_p, hop = _setup(dev, model[1], target, solver)
    eager, replayed, h_e, h_g = _both(eng, canvas_p, hop, SCHED4, n_slots, SEED)
    assert replayed.shape == eager.shape and torch.isfinite(replayed).all() and float(replayed.std()) > 0
    assert torch.equal(replayed, eager), float((replayed - eager).abs().max())
    if solver == "dpmpp_2m":
        assert torch.equal(h_g, h_e)
    else:
        assert h_e is None and h_g is None


@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
def test_fifo_denoise_graph_replays_two_ramp_pairs(dev, model, solver):
    """n = 6 (B = 3, S = 2): five ramp steps = one eager step and two replays of the pair; graph=None takes the replay here (2 * 3 * N
    rows is far below GRAPH_BELOW_ROWS)"""
    eng, canvas_p, hop = _setup(dev, model[1], "video", solver, B=3)
    assert 2 * 3 * eng.N < eng.GRAPH_BELOW_ROWS
    for graph in (True, None):
        eager, replayed, h_e, h_g = _both(eng, canvas_p, hop, SCHED6, 4, SEED, graph=graph)
        assert torch.equal(replayed, eager), graph
        if solver == "dpmpp_2m":
            assert torch.equal(h_g, h_e), graph


# ------------------------------------------------------------------------------------------------- 6. no stale by-value state
@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
def test_graph_calls_on_one_engine_hold_nothing_stale(dev, model, solver):
    import multimodal_diffusion_amd as A
    eng, canvas_p, hop = _setup(dev, model[1], "video", solver)
    ref, _, _ = _setup(dev, model[1], "video", solver)              # the eager results come from an engine of their own
    canvas_2 = torch.randn(canvas_p.shape, generator=torch.Generator().manual_seed(99)).to(dev)
    seen = []
    for seed, K, pc in ((SEED, 4, canvas_p), (SEED + 1, 4, canvas_p), (SEED, 7, canvas_p), (SEED, 7, canvas_2)):
        out = A.fifo_denoise(eng, pc, hop, SCHED4, K, seed, graph=True)
        assert torch.equal(out, A.fifo_denoise(ref, pc, hop, SCHED4, K, seed)), (seed, K)
        seen.append(out)
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[2], seen[3])
    assert torch.equal(seen[2][:, :seen[0].shape[1]], seen[0])     # the longer clip of seed A starts as the shorter one
    # an earlier call's canvas is its caller's: the later calls did not write it
    assert torch.equal(seen[0], A.fifo_denoise(ref, canvas_p, hop, SCHED4, 4, SEED))


# ------------------------------------------------------------------------------------------------- 7. refusals
def _raised(fn):
    with pytest.raises(Exception) as e:
        fn()
    return type(e.value), str(e.value)


def test_graph_refuses_what_the_eager_call_refuses(dev, model):
    import multimodal_diffusion_amd as A
    good, canvas_p, hop = _setup(dev, model[1], "video", "ddim")
    stochastic = engine(model[1], "video", (2, 8, 4, 16, 16), 10, guidance=GS, eta=0.5)
    guided = engine(model[1], "video", (2, 8, 4, 16, 16), 10, guidance=GS)
    guided.set_known(torch.zeros(2, 8, 4, 16, 16, device=dev))
    cases = [(stochastic, SCHED4, ValueError, "eta == 0"), (guided, SCHED4, ValueError, "latent guide"),
             (good, torch.tensor([999, 499, -1]), ValueError, "queue")]
    for eng, sched, kind, words in cases:
        eager = _raised(lambda: A.fifo_denoise(eng, canvas_p, hop, sched, 4, SEED))
        replayed = _raised(lambda: A.fifo_denoise(eng, canvas_p, hop, sched, 4, SEED, graph=True))
        assert eager == replayed and eager[0] is kind and words in eager[1], (eager, replayed)
        assert not torch.cuda.is_current_stream_capturing()
        # and a following eager call works
        assert torch.isfinite(A.fifo_denoise(good, canvas_p, hop, SCHED4, 2, SEED)).all()
    guided.clear_known()
    assert torch.equal(A.fifo_denoise(guided, canvas_p, hop, SCHED4, 2, SEED, graph=True), A.fifo_denoise(good, canvas_p, hop, SCHED4, 2, SEED))
    # graph is True, False or None
    for bad in (1, 0, "yes", 1.0):
        with pytest.raises(TypeError, match="graph"):
            A.fifo_denoise(good, canvas_p, hop, SCHED4, 2, SEED, graph=bad)
