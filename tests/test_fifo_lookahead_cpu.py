"""CPU tests of FIFO lookahead denoising: the plan's timestep tables against their definitions and their properties, the generalised
prompt windows, the reference's own queue map, and the bindings and refusals of the two lookahead entries."""
import re
from pathlib import Path

import pytest
import torch

import _lookahead_ref as LR

ROOT = Path(__file__).resolve().parent.parent
NEW = ("avd_fifo_lookahead_f32", "avd_fifo_lookahead_hist_f32")
CASES = [(4, 2, 3), (4, 1, 2), (4, 3, 3), (2, 1, 2)]          # (S, ctx, B)


def _sched(n):
    """s_0 > ... > s_n = -1"""
    return torch.linspace(999, -1, n + 1).round().long()


def _tables(S, ctx, B, context):
    from multimodal_diffusion_amd import schedule_utils as su
    sched = _sched(B * (S - ctx))
    rn, rp, sn, sp = su.fifo_lookahead_plan(sched, S, ctx, context)
    rl, sl = su.fifo_lookahead_plan_last(sched, S, ctx, context)
    return sched.tolist(), (rn, rp, rl, sn, sp, sl)


# ------------------------------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("context", ["noise", "clean"])
@pytest.mark.parametrize("S,ctx,B", CASES)
def test_plan_equals_its_definition(S, ctx, B, context):
    s, got = _tables(S, ctx, B, context)
    n = B * (S - ctx)
    ref = LR.plan(s, S, ctx, context)
    for name, g, r, rows in zip(("ramp_now", "ramp_prev", "ramp_last", "steady_now", "steady_prev", "steady_last"), got, ref,
                                (n - 1,) * 3 + (ctx + 1,) * 3):
        assert g.dtype == torch.long and g.shape == (rows, B, S), name
        assert torch.equal(g, r), name


@pytest.mark.parametrize("context", ["noise", "clean"])
@pytest.mark.parametrize("S,ctx,B", CASES)
def test_every_active_slot_takes_every_step_in_order(S, ctx, B, context):
    s, (rn, rp, rl, sn, sp, sl) = _tables(S, ctx, B, context)
    h = S - ctx
    n = B * h
    at = lambda t, row, a: int(t[row][LR.owner(ctx + a, S, ctx)])         # the owner copy of active slot a
    for K in (1, n, n + 3):
        for c in range(K):
            triples = []
            if c < n:                                   # in the initial queue at active slot c: the whole ramp, no shift
                triples += [(at(rn, r, c), at(rp, r, c), at(rl, r, c)) for r in range(n - 1)]
            # steady iteration m: clip slot c sits at active slot c - m
            triples += [(at(sn, min(m, ctx), c - m), at(sp, min(m, ctx), c - m), at(sl, min(m, ctx), c - m))
                        for m in range(max(0, c - n + 1), c + 1)]
            steps = [t for t in triples if t[0] != t[1]]
            assert [t[:2] for t in steps] == [(s[i], s[i + 1]) for i in range(n)], (K, c, triples)
            assert [t[2] for t in steps] == [-1] + s[:n - 1]              # every step's history is its previous step's
            assert all(t == (s[0], s[0], -1) for t in triples if t[0] == t[1])
            assert triples[-1][1] == -1


@pytest.mark.parametrize("context", ["noise", "clean"])
@pytest.mark.parametrize("S,ctx,B", CASES)
def test_duplicates_are_held_at_their_owners_timestep(S, ctx, B, context):
    s, (rn, rp, rl, sn, sp, sl) = _tables(S, ctx, B, context)
    h = S - ctx
    n = B * h
    for now, prev, last in ((rn, rp, rl), (sn, sp, sl)):
        for row in range(now.shape[0]):
            for k in range(B):
                for p in range(S):
                    own = int(now[row][LR.owner(k * h + p, S, ctx)])
                    assert int(now[row, k, p]) == own                    # every copy of a slot embeds one timestep
                    if p < ctx:                                          # held, and exactly the first ctx of every window ...
                        assert int(prev[row, k, p]) == own and int(last[row, k, p]) == -1
                    elif now is sn:                                      # ... in the steady state every other position steps
                        assert int(prev[row, k, p]) < own
    # in the ramp a stepping position holds only while its slot waits, at s_0
    for r in range(n - 1):
        for a in range(n):
            k, p = LR.owner(ctx + a, S, ctx)
            assert (int(rp[r, k, p]) == int(rn[r, k, p])) == (a > r)
    # steady rows differ only in the context slots' entries, which end up clean: window 0's first ctx positions — and, where ctx > h
    # puts a context slot into later windows too, its duplicates there, which the invariant above ties to window 0's entry
    q = torch.arange(B)[:, None] * h + torch.arange(S)[None, :]
    for t in (sn, sp, sl):
        assert all(torch.equal(t[row][q >= ctx], t[0][q >= ctx]) for row in range(ctx + 1))
        if ctx <= h:
            assert all(torch.equal(t[row][1:], t[0][1:]) and torch.equal(t[row][0, ctx:], t[0][0, ctx:]) for row in range(ctx + 1))
    assert (sn[ctx][0, :ctx] == 0).all()
    lab = s[0] if context == "noise" else 0
    assert (sn[0][0, :ctx] == lab).all() and (rn[:, 0, :ctx] == lab).all()


def test_ctx_0_is_fifo_plan():
    from multimodal_diffusion_amd import schedule_utils as su
    sched = _sched(6)
    rn, rp, sn, sp = su.fifo_plan(sched, 3)
    rl, sl = su.fifo_plan_last(sched, 3)
    got = su.fifo_lookahead_plan(sched, 3, 0) + su.fifo_lookahead_plan_last(sched, 3, 0)
    for g, r in zip(got, (rn, rp, sn[None], sp[None], rl, sl[None])):
        assert g.shape == r.shape and torch.equal(g, r)
    assert got[2].shape == (1, 2, 3)


def test_plan_refusals():
    from multimodal_diffusion_amd import schedule_utils as su
    for f in (su.fifo_lookahead_plan, su.fifo_lookahead_plan_last):
        with pytest.raises(ValueError, match="strictly decreasing"):
            f(torch.tensor([900, 500, 500, 100, -1]), 4, 2)
        with pytest.raises(ValueError, match="ends in -1"):
            f(torch.tensor([900, 500, 100, 0]), 4, 1)
        with pytest.raises(ValueError, match="multiple"):
            f(_sched(5), 4, 2)                                            # n = 5, h = 2
        with pytest.raises(ValueError, match="ctx"):
            f(_sched(4), 4, 4)
        with pytest.raises(ValueError, match="ctx"):
            f(_sched(4), 4, -1)
        with pytest.raises(ValueError, match="context"):
            f(_sched(4), 4, 2, "dirty")


# ------------------------------------------------------------------------------------------------- the reference's own map
@pytest.mark.parametrize("S,ctx,B", CASES)
def test_reference_map_tiles_the_queue(S, ctx, B):
    h = S - ctx
    Q = ctx + B * h
    owners = [LR.owner(q, S, ctx) for q in range(Q)]
    assert len(set(owners)) == Q and all(k * h + p == q for q, (k, p) in enumerate(owners))
    assert sorted(o for o in owners[ctx:]) == [(k, p) for k in range(B) for p in range(ctx, S)]      # stepping slots tile the active queue
    old = [torch.full((2, 1), float(q)) for q in range(Q)]
    z = LR.windows(old, B, S, ctx)
    assert LR.coherent(z, ctx, 1) and [float(o[0, 0]) for o in LR.logical(z, ctx, 1)] == list(range(Q))
    z1, popped = LR.lookahead(z, ctx, 1, 1, torch.full((2, 1), float(Q)))
    assert float(popped[0, 0]) == ctx and [float(o[0, 0]) for o in LR.logical(z1, ctx, 1)] == list(range(1, Q + 1))
    z[1, :, 0] = -1.0                                                      # a stale duplicate ...
    assert ctx == 0 or not LR.coherent(z, ctx, 1)
    assert LR.coherent(LR.lookahead(z, ctx, 0, 1)[0], ctx, 1)              # ... is refreshed from its owner


# ------------------------------------------------------------------------------------------------- prompt windows
def test_fifo_prompt_windows_stride_and_first():
    from multimodal_diffusion_amd.stream_infer import fifo_prompt_windows
    B, S, hop, Lp = 3, 4, 3, 8
    audio = torch.arange(1, 2 * 17 + 1, dtype=torch.float32).view(2, 17)                   # [Ca, P]
    video = torch.arange(1, 2 * 17 * 6 + 1, dtype=torch.float32).view(2, 17, 2, 3)         # [C, P, H, W]
    for canvas in (audio, video):
        for m in (0, 1, 4):
            # the defaults reproduce the current output
            assert torch.equal(fifo_prompt_windows(canvas, m, B, S, hop, Lp), LR.prompt_windows(canvas, m, B, S, hop, Lp))
            assert torch.equal(fifo_prompt_windows(canvas, m, B, S, hop, Lp, stride=S, first=m), fifo_prompt_windows(canvas, m, B, S, hop, Lp))
            for ctx in (1, 2, 3):
                w = fifo_prompt_windows(canvas, m, B, S, hop, Lp, stride=S - ctx, first=m - ctx)
                assert torch.equal(w, LR.prompt_windows(canvas, m - ctx, B, S - ctx, hop, Lp))
    w = fifo_prompt_windows(audio, 0, B, S, hop, Lp, stride=2, first=-2)
    assert (w[0, :, :6] == 0).all() and torch.equal(w[0, :, 6:], audio[:, :2])            # negative positions give zeros
    assert (fifo_prompt_windows(audio, 0, B, S, hop, Lp, stride=1, first=-3)[0] == 0).all()
    with pytest.raises(ValueError):
        fifo_prompt_windows(audio, 0, B, S, hop, Lp, stride=0)


# ------------------------------------------------------------------------------------------------- bindings
def test_lookahead_entries_declared_exported_and_bound():
    from multimodal_diffusion_amd import _lib as L
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import functional as Fn
    header = (ROOT / "include" / "avdiff_hip.h").read_text()
    declared = set(re.findall(r"\b(avd_[a-z0-9_]+)\s*\(", header))
    lib = L.lib()
    for name in NEW:
        assert name in declared and name in L.SIGNATURES and hasattr(lib, name), name
    assert lib.avd_abi_version() == L.ABI_VERSION == 7
    assert "FIFO lookahead" in header
    assert callable(Fn.fifo_lookahead) and hasattr(A.DenoiseEngine, "fifo_lookahead")


def test_lookahead_entries_refuse_before_any_launch():
    """argument checks run before any HIP call, so a CPU-only machine sees them"""
    import ctypes as C
    from multimodal_diffusion_amd import _lib as L
    lib = L.lib()
    p = 4096                                             # a non-null, 16-byte aligned stand-in: nothing is dereferenced
    key = C.byref(L.NoiseKey(7, 0))
    big = 1 << 30
    dims = lambda ctx, slots=4: (2, 8, slots, ctx, 2, 256, None)          # B, outer, slots, ctx, slot_len, inner, stream
    f, fh = lib.avd_fifo_lookahead_f32, lib.avd_fifo_lookahead_hist_f32
    for ctx in (4, 5, -1):
        assert f(key, 999, 4, 1, p, 2 * big, 3 * big, *dims(ctx)) == L.EINVAL
        assert b"ctx" in lib.avd_last_error()
    for shift in (2, -1):
        assert f(key, 999, 4, shift, p, 2 * big, 3 * big, *dims(2)) == L.EINVAL
        assert b"shift" in lib.avd_last_error()
    assert f(None, 0, 0, 0, p, 2 * big, 3 * big, *dims(2)) == L.EINVAL                    # popped at shift 0
    assert b"popped must be null" in lib.avd_last_error()
    assert f(key, 999, 4, 1, p, 2 * big, None, *dims(2)) == L.EINVAL                      # no popped at shift 1
    assert f(None, 999, 4, 1, p, 2 * big, 3 * big, *dims(2)) == L.EINVAL                  # no key at shift 1
    assert f(key, 999, 2 ** 31, 1, p, 2 * big, 3 * big, *dims(2)) == L.EINVAL
    assert b"2^32" in lib.avd_last_error()
    for shift, popped in ((1, 3 * big), (0, None)):
        assert f(key, 999, 4, shift, p, p + 64, popped, *dims(2)) == L.EINVAL
        assert b"z_out must not overlap z_in" in lib.avd_last_error()
    assert f(key, 999, 4, 1, p, 2 * big, p + 64, *dims(2)) == L.EINVAL
    assert b"popped must not overlap" in lib.avd_last_error()
    # the history pair: both set, apart from each other, from the latents and from popped
    assert fh(key, 999, 4, 1, p, 2 * big, 3 * big, None, 5 * big, *dims(2)) == L.EINVAL
    assert fh(key, 999, 4, 1, p, 2 * big, 3 * big, 4 * big, 4 * big + 64, *dims(2)) == L.EINVAL
    assert b"hist_out must not overlap hist_in" in lib.avd_last_error()
    assert fh(None, 0, 0, 0, p, 2 * big, None, 4 * big, p + 64, *dims(2)) == L.EINVAL
    assert b"hist_in and hist_out must not overlap z_in or z_out" in lib.avd_last_error()
    assert fh(key, 999, 4, 1, p, 2 * big, 4 * big + 64, 4 * big, 5 * big, *dims(2)) == L.EINVAL
    assert b"popped must not overlap hist_in" in lib.avd_last_error()
    assert fh(key, 999, 4, 1, p, 2 * big, 3 * big, 4 * big, 5 * big, *dims(4)) == L.EINVAL
    assert b"ctx" in lib.avd_last_error()
