"""Clip batch keying on the GPU (include/avdiff_hip.h, "clip batch keying"): per-queue step noise and per-queue latent guides of a FIFO
clip batch.  The reference of every comparison is the existing one-queue entry on the K sample slices, so every comparison is
``torch.equal``: the fused updates through the C entries (both solvers, both video forms, the audio form), the guide's properties, the
stand-alone passes, K = 1, the whole step, ``fifo_denoise_clips(step_seeds=, init_canvases=)``, one pipeline call, and the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from _kit import ABAR, audio_prompt, components, dev, engine, model, pipeline  # noqa: F401  (dev, model are fixtures)
from _tune import tuned

pytestmark = pytest.mark.gpu

GS, T_TRAIN = 3.5, 1000
SEEDS = [0x5EED0F1F0, 2 ** 64 - 3, 11]          # step seeds: one above 2^63
GSEEDS = [5, 2 ** 63 + 9, 5]                    # guide seeds: a duplicate
SCHED4 = [999, 749, 499, 249, -1]
# (target, batch shape, patch, K): the shapes of test_gpu_fifo_clips.py; B_q = 2, B_q = 1, and the audio form (the scalar lane)
GEOMS = [("video", (4, 8, 4, 16, 16), (2, 4, 4), 2), ("video", (3, 8, 4, 16, 16), (2, 4, 4), 3), ("audio", (6, 8, 8), (4, 4), 3)]
UPDATES = [(0.5, False), (0.5, True)]           # DDIM at eta 0.5, the SDE form of DPM-Solver++(2M)
FIRSTS = [0, 3, -2]


def _fn():
    from multimodal_diffusion_amd import _lib as L
    from multimodal_diffusion_amd import functional as Fn
    return L, Fn


def _dims(geom):
    target, shape, patch, K = geom
    video = target == "video"
    sl = patch[0]
    S = shape[2] // sl
    Nt = S * (shape[3] // patch[1]) * (shape[4] // patch[2]) if video else S
    D = shape[1] * patch[0] * patch[1] * patch[2] if video else shape[1] * patch[0]
    return video, sl, S, Nt, D


def _tables(B, S, dev):
    """[B, S] tables that mix stepping slots, held slots and a final step to -1 (and first- and second-order histories)"""
    pat = [(749, 499, 999), (499, 499, -1), (249, -1, 499), (999, 749, -1), (499, 249, 749)]
    rows = [pat[(b * S + s) % len(pat)] for b in range(B) for s in range(S)]
    tn, tp, tl = (torch.tensor([r[i] for r in rows], dtype=torch.long, device=dev).view(B, S) for i in range(3))
    return tn, tp, tl


def _inputs(geom, dev, seed=0):
    video, sl, S, Nt, D = _dims(geom)
    shape, B = geom[1], geom[1][0]
    g = torch.Generator().manual_seed(sum(shape) + seed)
    z, hist = (torch.randn(shape, generator=g).to(dev) for _ in range(2))
    eps2 = torch.randn(2 * B, Nt, D, generator=g).to(dev)
    return z, eps2, hist


def _canvases(geom, dev, P=None, seed=1, offset=0):
    """(known [K, C, P, ...], soft masks) with P = 5.5 slots: the last slot of a queue of two samples at first = 0 under a cursor of 2
    straddles the canvas end.  ``offset`` = 1 puts both one float off a 16-byte boundary."""
    _, shape, patch, K = geom
    P = patch[0] * 5 + patch[0] // 2 if P is None else P
    cs = (K, shape[1], P) + tuple(shape[3:])
    g = torch.Generator().manual_seed(seed + len(shape))
    known = torch.randn(cs, generator=g)
    m = torch.rand(cs, generator=g)
    m = torch.where(m < 0.3, torch.zeros(()), torch.where(m > 0.7, torch.ones(()), m))
    outs = []
    for t in (known, m):
        buf = torch.empty(t.numel() + 4, device=dev)
        outs.append(buf[offset:offset + t.numel()].view(cs).copy_(t))
        assert outs[-1].data_ptr() % 16 == 4 * offset
    return outs


def _run(dev, geom, z, eps2, tn, tp, tl, hist, eta, key, guide, cq=None, ctl=None):
    """one fused update through a C entry: the clips entry with ``cq``, else the existing controlled (``ctl``: an avd_slot_cfg), guided
    or seeded entry"""
    L, _ = _fn()
    video, sl, S, Nt, D = _dims(geom)
    out = torch.empty_like(z)
    ab = ABAR.to(dev, torch.float32)
    name = "avd_cfg_unpatch_ddim" if video else "avd_cfg_untoken_ddim_audio"
    head = (eps2.data_ptr(), z.data_ptr(), L.ptr(tl), tn.data_ptr(), tp.data_ptr(), ab.data_ptr(), T_TRAIN, GS, eta)
    dims = (z.shape[0],) + tuple(geom[1][1:]) + tuple(geom[2])
    kp, gp = (None if key is None else C.byref(key)), (None if guide is None else C.byref(guide))
    cp = None if ctl is None else C.byref(ctl)
    st = L.stream_ptr(dev)
    if cq is not None:
        rc = getattr(L.lib(), name + "_slots_clips_f32")(*head, kp, gp, C.byref(cq), S, L.ptr(hist), out.data_ptr(), *dims, cp, st)
    elif ctl is not None:
        rc = getattr(L.lib(), name + "_slots_cfg_f32")(*head, kp, gp, S, L.ptr(hist), out.data_ptr(), *dims, cp, st)
    elif guide is not None:
        rc = getattr(L.lib(), name + "_slots_guided_f32")(*head, kp, gp, S, L.ptr(hist), out.data_ptr(), *dims, st)
    else:
        rc = getattr(L.lib(), name + "_slots_seeded_f32")(*head, kp, S, L.ptr(hist), out.data_ptr(), *dims, st)
    L.check(rc)
    return out, ab


def _queues(dev, K, B, step=None, guide=None):
    """(avd_clip_queues, the tensors it points to)"""
    _, Fn = _fn()
    s = None if step is None else Fn.queue_seeds(step, K, dev)
    g = None if guide is None else Fn.queue_seeds(guide, K, dev)
    return Fn.clip_queues(K, B, s, g), (s, g)


def _clips(dev, geom, z, eps2, tn, tp, tl, hist, eta, first, cursor, step=None, known=None, masks=None, gseeds=None, K=None, ctl=None):
    """the clips entry on the whole batch: (z_out, x0_hist after); ``ctl``: samples -> the batch's avd_slot_cfg"""
    _, Fn = _fn()
    _, sl, S, _, _ = _dims(geom)
    K = geom[3] if K is None else K
    key = Fn.slot_key(0, first, S, cursor, dev) if eta > 0 else None
    guide = None if known is None else Fn.clip_guide(known[0], None if masks is None else masks[0], 0, first, S, cursor, tuple(z.shape))
    cq, keep = _queues(dev, K, z.shape[0], step if eta > 0 else None, gseeds if known is not None else None)
    h = None if hist is None else hist.clone()
    out, _ = _run(dev, geom, z, eps2, tn, tp, tl if h is not None else None, h, eta, key, guide, cq,
                  None if ctl is None else ctl(slice(0, z.shape[0])))
    return out, h


def _slices(dev, geom, z, eps2, tn, tp, tl, hist, eta, first, cursor, step, known=None, masks=None, gseeds=None, K=None, ctl=None):
    """the reference: K calls of the existing seeded / guided / controlled entry on the K sample slices"""
    _, Fn = _fn()
    _, sl, S, _, _ = _dims(geom)
    K = geom[3] if K is None else K
    B = z.shape[0]
    Bq = B // K
    out = torch.empty_like(z)
    h_out = None if hist is None else hist.clone()
    for k in range(K):
        q = slice(k * Bq, (k + 1) * Bq)
        key = Fn.slot_key(step[k], first, S, cursor, dev)
        guide = None
        if known is not None:
            guide = Fn.clip_guide(known[k], None if masks is None else masks[k], gseeds[k], first, S, cursor, (Bq,) + tuple(z.shape[1:]))
        e = torch.cat([eps2[:B][q], eps2[B:][q]]).contiguous()
        h = None if hist is None else hist[q].clone()
        out[q], _ = _run(dev, geom, z[q].contiguous(), e, tn[q].contiguous(), tp[q].contiguous(),
                         tl[q].contiguous() if h is not None else None, h, eta, key, guide, ctl=None if ctl is None else ctl(q))
        if h is not None:
            h_out[q] = h
    return out, h_out


def _same(a, b):
    assert torch.equal(a[0], b[0]), float((a[0] - b[0]).abs().max())
    assert (a[1] is None) == (b[1] is None) and (a[1] is None or torch.equal(a[1], b[1]))


# ------------------------------------------------------------------------------------------------- 1. the fused updates
@pytest.mark.parametrize("first", FIRSTS)
@pytest.mark.parametrize("eta,dpm", UPDATES)
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: f"{g[0]}{g[1][0]}k{g[3]}")
def test_fused_updates_equal_the_one_queue_entries_on_slices(dev, geom, eta, dpm, first):
    K, B = geom[3], geom[1][0]
    _, sl, S, _, _ = _dims(geom)
    z, eps2, hist = _inputs(geom, dev)
    tn, tp, tl = _tables(B, S, dev)
    assert bool((tn == tp).any()) and bool((tp == -1).any()) and bool((tn != tp).any())
    cursor = torch.tensor([2], dtype=torch.int32, device=dev)
    known, masks = _canvases(geom, dev)
    h0 = hist if dpm else None
    for rows in ((1, 0) if geom[0] == "video" else (1,)):
        with tuned(cfg_rows=rows):
            # per-queue keys alone
            got = _clips(dev, geom, z, eps2, tn, tp, tl, h0, eta, first, cursor, step=SEEDS[:K])
            _same(got, _slices(dev, geom, z, eps2, tn, tp, tl, h0, eta, first, cursor, SEEDS[:K]))
            # keys and guides together; the guide alone at eta == 0 (the key is then not read, and may be null)
            for e in (eta, 0.0):
                gg = _clips(dev, geom, z, eps2, tn, tp, tl, h0, e, first, cursor, step=SEEDS[:K], known=known, masks=masks, gseeds=GSEEDS[:K])
                _same(gg, _slices(dev, geom, z, eps2, tn, tp, tl, h0, e, first, cursor, SEEDS[:K], known, masks, GSEEDS[:K]))
                assert not torch.equal(gg[0], got[0])
            # the queues draw apart: the one-queue entry under seed 0 on the whole batch is something else
            whole = _slices(dev, geom, z, eps2, tn, tp, tl, h0, eta, first, cursor, SEEDS[:1], K=1)
            Bq = B // K
            assert torch.equal(whole[0][:Bq], got[0][:Bq]) and not torch.equal(whole[0][Bq:], got[0][Bq:])


def test_canvases_off_a_16_byte_boundary_take_the_scalar_reads(dev):
    geom = GEOMS[0]
    z, eps2, hist = _inputs(geom, dev)
    tn, tp, tl = _tables(4, 2, dev)
    cursor = torch.tensor([2], dtype=torch.int32, device=dev)
    known, masks = _canvases(geom, dev)
    ku, mu = _canvases(geom, dev, offset=1)
    assert torch.equal(ku, known) and ku.data_ptr() % 16 == 4
    for rows in (1, 0):
        with tuned(cfg_rows=rows):
            a = _clips(dev, geom, z, eps2, tn, tp, tl, hist, 0.5, 0, cursor, step=SEEDS[:2], known=known, masks=masks, gseeds=GSEEDS[:2])
            b = _clips(dev, geom, z, eps2, tn, tp, tl, hist, 0.5, 0, cursor, step=SEEDS[:2], known=ku, masks=mu, gseeds=GSEEDS[:2])
            _same(a, b)
            _same(b, _slices(dev, geom, z, eps2, tn, tp, tl, hist, 0.5, 0, cursor, SEEDS[:2], ku, mu, GSEEDS[:2]))


WIDEST = [("video", (2, 8, 4, 16, 16), (2, 4, 4), 2), ("audio", (2, 6, 10), (4, 4), 2)]


@pytest.mark.parametrize("geom", WIDEST, ids=["video", "audio"])
def test_the_widest_slot_pack_equals_its_one_queue_slices(dev, geom):
    """DPM-Solver++(2M) at eta > 0 under a slot key, the slot APG with a momentum buffer, a masked clip guide and K = 2 queues: every
    item a slot pack can hold, in one launch of each form.  Slot 1 of sample 0 is held; with first + cursor = 4 and P = 5.5 slots the
    canvas ends inside every sample's second slot."""
    L, _ = _fn()
    video, sl, S, _, _ = _dims(geom)
    shape = geom[1]
    B, K = shape[0], geom[3]
    per_slot = shape[1] * sl * (shape[3] * shape[4] if video else 1)
    z, eps2, hist = _inputs(geom, dev, seed=5)
    tn, tp, tl = _tables(B, S, dev)
    held = (tn == tp).cpu()
    assert S == 2 and held.tolist() == [[False, True], [False, False]]
    cursor = torch.tensor([2], dtype=torch.int32, device=dev)
    known, masks = _canvases(geom, dev)
    assert (2 + 2) * sl < known.shape[2] < (2 + 2 + S) * sl
    M0 = torch.randn(shape, generator=torch.Generator().manual_seed(17)).to(dev)
    gtab = torch.linspace(1.0, 6.0, T_TRAIN).to(dev)
    keep = []

    def control(M):
        def of(q):
            n = q.stop - q.start
            nb = L.lib().avd_slot_cfg_stats_bytes(n, S, per_slot)
            stats = torch.zeros(nb, dtype=torch.uint8, device=dev)
            keep.append(stats)
            return L.SlotCfgMomentum(gtab.data_ptr(), None, L.SLOT_APG_MOMENTUM, 2.0, 0.25, stats.data_ptr(), nb, -0.5, M[q].data_ptr())
        return of

    got = {}
    for rows in ((1, 0) if video else (1,)):
        with tuned(cfg_rows=rows):
            Mk, Ms = M0.clone(), M0.clone()
            a = _clips(dev, geom, z, eps2, tn, tp, tl, hist, 0.5, 2, cursor, step=SEEDS[:K], known=known, masks=masks, gseeds=GSEEDS[:K],
                       ctl=control(Mk))
            _same(a, _slices(dev, geom, z, eps2, tn, tp, tl, hist, 0.5, 2, cursor, SEEDS[:K], known, masks, GSEEDS[:K], ctl=control(Ms)))
            assert torch.equal(Mk, Ms) and not torch.equal(Mk, M0)
            got[rows] = a + (Mk,)
    if video:
        assert all(torch.equal(x, y) for x, y in zip(got[1], got[0]))
    out, h, M = got[1]
    for b, s in held.nonzero().tolist():      # a held slot keeps z, and its history and momentum stay as they were
        for after, before in ((out, z), (h, hist), (M, M0)):
            assert torch.equal(after[b, :, s * sl:(s + 1) * sl], before[b, :, s * sl:(s + 1) * sl])
    assert not torch.equal(out[0, :, :sl], z[0, :, :sl])


# ------------------------------------------------------------------------------------------------- 2. the guide's properties
@pytest.mark.parametrize("eta,dpm", UPDATES + [(0.0, True)])
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: f"{g[0]}{g[1][0]}k{g[3]}")
def test_guide_properties(dev, geom, eta, dpm):
    K, B = geom[3], geom[1][0]
    Bq = B // K
    _, sl, S, _, _ = _dims(geom)
    z, eps2, hist = _inputs(geom, dev, seed=3)
    tn, tp, tl = _tables(B, S, dev)
    cursor = torch.tensor([2], dtype=torch.int32, device=dev)
    known, soft = _canvases(geom, dev)
    P = known.shape[2]
    h0 = hist if dpm else None
    args = (dev, geom, z, eps2, tn, tp, tl, h0, eta, 0, cursor)
    free = _clips(*args, step=SEEDS[:K])
    # positions: queue 1's last slot straddles the canvas end where a queue has two samples
    if Bq == 2:
        lo = (2 + S) * sl + (S - 1) * sl
        assert lo < P < lo + sl
    held = (tn == tp).repeat_interleave(sl, 1)                                    # [B, L]
    for masks in (soft, None, torch.zeros_like(soft)):
        got = _clips(*args, step=SEEDS[:K], known=known, masks=masks, gseeds=GSEEDS[:K])
        _same(got, _slices(*args, SEEDS[:K], known, masks, GSEEDS[:K]))
        # a held slot keeps z bit for bit, and its x0_hist is untouched; the history receives the unblended x0
        zt, ot = z.movedim(2, 1), got[0].movedim(2, 1)                            # [B, L, C, ...]
        assert torch.equal(ot[held], zt[held])
        if dpm:
            assert torch.equal(got[1].movedim(2, 1)[held], hist.movedim(2, 1)[held])
            assert torch.equal(got[1], free[1]) and not torch.equal(got[1], hist)
        if masks is not None and not bool(masks.any()):
            _same(got, free)                                                      # the all-zero mask: the unguided bits
        else:
            assert not torch.equal(got[0], free[0])
        if masks is None:                                                         # m == 1: a final step returns known[k] bit for bit
            n_final = 0
            for b in range(B):
                k, bq = divmod(b, Bq)
                for s in range(S):
                    if int(tp[b, s]) != -1 or int(tn[b, s]) == -1:
                        continue
                    for j in range(sl):
                        p = (0 + 2 + bq * S) * sl + s * sl + j
                        if 0 <= p < P:
                            assert torch.equal(got[0][b][:, s * sl + j], known[k][:, p])
                            n_final += 1
            assert n_final > 0
    # different guide seeds per queue: the duplicate seed of queue 2 against queue 0 is covered by the slices; swapping two changes bits
    sw = _clips(*args, step=SEEDS[:K], known=known, masks=soft, gseeds=[GSEEDS[1], GSEEDS[0]] + GSEEDS[2:K])
    ref = _clips(*args, step=SEEDS[:K], known=known, masks=soft, gseeds=GSEEDS[:K])
    assert not torch.equal(sw[0][:Bq], ref[0][:Bq])


# ------------------------------------------------------------------------------------------------- 3. the stand-alone passes
@pytest.mark.parametrize("first", FIRSTS)
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: f"{g[0]}{g[1][0]}k{g[3]}")
def test_stand_alone_passes_equal_the_one_queue_functions_on_slices(dev, geom, first):
    L, Fn = _fn()
    K, B, shape = geom[3], geom[1][0], geom[1]
    Bq = B // K
    _, sl, S, _, _ = _dims(geom)
    tn, tp, _ = _tables(B, S, dev)
    cursor = torch.tensor([2], dtype=torch.int32, device=dev)
    for cur in (cursor, None):                                                    # None at first = -2: negative positions wrap
        got = Fn.slot_noise_clips(SEEDS[:K], tn, shape, sl, first=first, cursor=cur)
        want = torch.cat([Fn.slot_noise(SEEDS[k], tn[k * Bq:(k + 1) * Bq], (Bq,) + shape[1:], sl, first=first, cursor=cur) for k in range(K)])
        assert torch.equal(got, want) and float(got.std()) > 0.5
        if K > 1:
            assert not torch.equal(got[:Bq], got[Bq:2 * Bq])
    # a misaligned out takes the guarded lanes (video) and the same bits; the CPU statement is the same map
    buf = torch.empty(got.numel() + 1, device=dev)[1:].view(shape)
    assert buf.data_ptr() % 16 != 0 and torch.equal(Fn.slot_noise_clips(SEEDS[:K], tn, shape, sl, first=first, cursor=None, out=buf), got)
    assert torch.equal(Fn.slot_noise_clips(SEEDS[:K], tn.cpu(), shape, sl, first=first, out=torch.empty(shape)), got.cpu())
    # the guide pass: out of place over every slot, in place over the K tails alone; aligned and one float off
    z = _inputs(geom, dev, seed=5)[0]
    ab = ABAR.to(dev, torch.float32)
    for offset in (0, 1):
        known, masks = _canvases(geom, dev, offset=offset)
        zz = torch.empty(z.numel() + 4, device=dev)[offset:offset + z.numel()].view(shape).copy_(z)
        for m, everywhere in ((masks, False), (None, False), (masks, True)):
            kw = dict(slot_len=sl, first=first, cursor=cursor, everywhere=everywhere)
            got = Fn.clip_guide_slots_clips(known, tn, ab, zz, m, seeds=GSEEDS[:K], **kw)
            want = torch.cat([Fn.clip_guide_slots(known[k], tn[k * Bq:(k + 1) * Bq], ab, z[k * Bq:(k + 1) * Bq].contiguous(),
                                                  None if m is None else m[k], seed=GSEEDS[k], **kw) for k in range(K)])
            assert torch.equal(got, want)
        tails = torch.full((B, S), Fn.SLOT_LEAVE, dtype=torch.long, device=dev)
        tails[Bq - 1::Bq, S - 1] = 999
        kw = dict(slot_len=sl, first=first, cursor=cursor)
        ip = zz.clone() if offset == 0 else torch.empty(z.numel() + 4, device=dev)[1:1 + z.numel()].view(shape).copy_(z)
        assert Fn.clip_guide_slots_clips(known, tails, ab, ip, masks, seeds=GSEEDS[:K], out=ip, **kw) is ip
        want = z.clone()
        for k in range(K):
            q = slice(k * Bq, (k + 1) * Bq)
            want[q] = Fn.clip_guide_slots(known[k], tails[q], ab, z[q].contiguous(), masks[k], seed=GSEEDS[k], **kw)
        assert torch.equal(ip, want)
        untouched = torch.ones(B, shape[2], dtype=torch.bool, device=dev)
        untouched[Bq - 1::Bq, (S - 1) * sl:S * sl] = False
        assert torch.equal(ip.movedim(2, 1)[untouched], z.movedim(2, 1)[untouched])
    # the CPU statement of the guide pass
    cpu = Fn.clip_guide_slots_clips(known.cpu(), tn.cpu(), ab, z.cpu(), masks.cpu(), slot_len=sl, seeds=GSEEDS[:K], first=first)
    dev_ = Fn.clip_guide_slots_clips(known.contiguous(), tn, ab, z, masks.contiguous(), slot_len=sl, seeds=GSEEDS[:K], first=first)
    assert torch.equal(cpu, dev_.cpu())


# ------------------------------------------------------------------------------------------------- 4. K == 1, equal queues, one seed moved
@pytest.mark.parametrize("eta,dpm", UPDATES)
@pytest.mark.parametrize("geom", [GEOMS[0], GEOMS[2]], ids=["video", "audio"])
def test_one_queue_is_the_existing_entry_and_queues_are_independent(dev, geom, eta, dpm):
    _, Fn = _fn()
    B = geom[1][0]
    _, sl, S, _, _ = _dims(geom)
    z, eps2, hist = _inputs(geom, dev, seed=7)
    tn, tp, tl = _tables(B, S, dev)
    cursor = torch.tensor([2], dtype=torch.int32, device=dev)
    h0 = hist if dpm else None
    one = (geom[0], geom[1], geom[2], 1)
    known, masks = _canvases(one, dev)
    a = _clips(dev, one, z, eps2, tn, tp, tl, h0, eta, 3, cursor, step=SEEDS[:1], known=known, masks=masks, gseeds=GSEEDS[:1])
    _same(a, _slices(dev, one, z, eps2, tn, tp, tl, h0, eta, 3, cursor, SEEDS[:1], known, masks, GSEEDS[:1]))
    # equal seeds and equal inputs in two queues give equal halves
    two = (geom[0], geom[1], geom[2], 2)
    Bq = B // 2
    dup = lambda t: torch.cat([t[:Bq], t[:Bq]]).contiguous()      # noqa: E731
    z2, tn2, tp2, tl2, h2 = dup(z), dup(tn), dup(tp), dup(tl), (dup(hist) if dpm else None)
    e2 = torch.cat([dup(eps2[:B]), dup(eps2[B:])]).contiguous()
    k2 = torch.cat([known, known]).contiguous()
    m2 = torch.cat([masks, masks]).contiguous()
    eq = _clips(dev, two, z2, e2, tn2, tp2, tl2, h2, eta, 3, cursor, step=[7, 7], known=k2, masks=m2, gseeds=[9, 9])
    assert torch.equal(eq[0][:Bq], eq[0][Bq:]) and (not dpm or torch.equal(eq[1][:Bq], eq[1][Bq:]))
    # changing step_seeds[1] changes queue 1 only
    mv = _clips(dev, two, z2, e2, tn2, tp2, tl2, h2, eta, 3, cursor, step=[7, 8], known=k2, masks=m2, gseeds=[9, 9])
    assert torch.equal(mv[0][:Bq], eq[0][:Bq]) and not torch.equal(mv[0][Bq:], eq[0][Bq:])


# ------------------------------------------------------------------------------------------------- 5. the whole step
def _engine(mods, target, B, **kw):
    if target == "video":
        return engine(mods, "video", (B, 8, 4, 16, 16), 10, guidance=GS, **kw)
    return engine(mods, "audio", (B, 8, 8), 8, guidance=GS, **kw)


@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
@pytest.mark.parametrize("target", ["video", "audio"])
def test_whole_step_equals_the_existing_step_per_queue(dev, model, target, solver):
    """samples never interact, so on one batch size queue 0 of the clip batch's step is the existing step under (a, f) and queue 1 the
    existing step under (b, f - B_q * stride)"""
    B, Bq, a, b = 4, 2, SEEDS[0], SEEDS[1]
    eng = _engine(model[1], target, B, eta=0.5, noise_seed=a, solver=solver)
    S, sl = eng.slots, eng.slot_len
    g = torch.Generator().manual_seed(23)
    z = torch.randn(eng.latent_shape, generator=g).to(dev)
    h0 = torch.randn(eng.latent_shape, generator=g).to(dev)
    prompt = torch.randn((B, 8, 40) if target == "video" else (B, 8, 4, 8, 8), generator=g).to(dev)
    eng.set_prompt(prompt)
    tn, tp, tl = _tables(B, S, dev)
    dpm = solver == "dpmpp_2m"

    def step(seed=None, **kw):
        if dpm:
            eng.x0_hist.copy_(h0)
        eng.noise_seed = seed
        out = eng.step_slots(z, tn, tp, t_last=tl if dpm else None, **kw)
        return out, (eng.x0_hist.clone() if dpm else None)

    geom = (target, tuple(eng.latent_shape), (2, 4, 4) if target == "video" else (4, 4), 2)
    known, masks = _canvases(geom, dev)
    for f in (3, -2):
        for guided in (False, True):
            if guided:
                eng.set_clip_guides(known, masks, guide_seeds=GSEEDS[:2])
            got = step(None, clip_first=f, clip_queues=2, clip_seeds=[a, b])      # the engine's own noise_seed is not read
            eng.clear_clip_guides()
            refs = []
            for k, (seed, first) in enumerate(((a, f), (b, f - Bq * S))):
                if guided:
                    eng.set_clip_guide(known[k], masks[k], guide_seed=GSEEDS[k])
                refs.append(step(seed, clip_first=first))
                eng.clear_clip_guide()
            for k in range(2):
                q = slice(k * Bq, (k + 1) * Bq)
                assert torch.equal(got[0][q], refs[k][0][q]), (f, guided, k)
                assert not dpm or torch.equal(got[1][q], refs[k][1][q])
            assert not torch.equal(got[0][Bq:], refs[0][0][Bq:])
    # the engine's refusals
    eng.noise_seed = a
    with pytest.raises(ValueError, match="pass clip_seeds"):
        eng.step_slots(z, tn, tp, t_last=tl if dpm else None, clip_first=0, clip_queues=2)
    with pytest.raises(ValueError, match="need clip_queues"):
        eng.step_slots(z, tn, tp, t_last=tl if dpm else None, clip_first=0, clip_seeds=[a, b])
    with pytest.raises(ValueError, match="divides the batch"):
        eng.step_slots(z, tn, tp, t_last=tl if dpm else None, clip_first=0, clip_queues=3, clip_seeds=[a, b, a])
    eng.set_clip_guides(known, masks, guide_seeds=GSEEDS[:2])
    with pytest.raises(ValueError, match="needs clip_queues"):
        eng.step_slots(z, tn, tp, t_last=tl if dpm else None, clip_first=0)
    for what, call in (("step", lambda: eng.step(z, tn[:, 0], tp[:, 0])), ("run", lambda: eng.run(z, torch.tensor(SCHED4)))):
        with pytest.raises(ValueError, match=f"{what} takes no clip guides"):
            call()
    eng.clear_clip_guides()
    eng.set_clip_guide(known[0])
    with pytest.raises(ValueError, match=r"step_slots\(clip_queues=\) takes no clip guide"):
        eng.step_slots(z, tn, tp, t_last=tl if dpm else None, clip_first=0, clip_queues=2, clip_seeds=[a, b])
    eng.clear_clip_guide()


# ------------------------------------------------------------------------------------------------- 6. the driver
def _setup(dev, mods, target, K, Bq, **kw):
    """test_gpu_fifo_clips.py's small queues: (engine of batch K * Bq, K prompt canvases, prompt_hop)"""
    g = torch.Generator().manual_seed(17)
    eng = _engine(mods, target, K * Bq, **kw)
    if target == "video":
        return eng, [torch.randn(8, 150, generator=g).to(dev) for _ in range(K)], 20
    return eng, [torch.randn(8, 14, 8, 8, generator=g).to(dev) for _ in range(K)], 2


def _clip_canvas(eng, n_slots, seed):
    """a clean clip canvas of n_slots slots and a mask that holds its second slot (1) and frees the rest"""
    cs = tuple(eng.latent_shape[1:2]) + (n_slots * eng.slot_len,) + tuple(eng.latent_shape[3:])
    c = torch.randn(cs, generator=torch.Generator().manual_seed(seed)).to(eng.device)
    m = torch.zeros(cs, device=eng.device)
    m[:, eng.slot_len:2 * eng.slot_len] = 1.0
    return c, m


@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
@pytest.mark.parametrize("target", ["video", "audio"])
def test_one_clip_is_fifo_denoise_at_eta_above_zero(dev, model, target, solver):
    import multimodal_diffusion_amd as A
    eng, pcs, hop = _setup(dev, model[1], target, 1, 2, solver=solver, eta=0.5, noise_seed=SEEDS[1])
    sched = torch.tensor(SCHED4)
    want = A.fifo_denoise(eng, pcs[0], hop, sched, 3, 31)
    eng.noise_seed = None                                                         # the step seeds stand in for it
    got = A.fifo_denoise_clips(eng, pcs, hop, sched, 3, [31], step_seeds=[SEEDS[1]])
    assert torch.equal(got[0], want)
    c, m = _clip_canvas(eng, 3, 4)
    eng.noise_seed = SEEDS[1]
    for start in ("noise", "init"):
        want = A.fifo_denoise(eng, pcs[0], hop, sched, 3, 31, init_canvas=c, mask=m, guide_seed=6, guide_start=start)
        got = A.fifo_denoise_clips(eng, pcs, hop, sched, 3, [31], step_seeds=[SEEDS[1]], init_canvases=[c], masks=[m], guide_seeds=[6],
                                   guide_start=start)
        assert torch.equal(got[0], want) and eng._clips is None
        assert torch.equal(got[0][:, eng.slot_len:2 * eng.slot_len], c[:, eng.slot_len:2 * eng.slot_len])


@pytest.mark.parametrize("target", ["video", "audio"])
def test_clips_are_independent_and_a_held_region_is_the_canvas(dev, model, target):
    import multimodal_diffusion_amd as A
    eng, pcs, hop = _setup(dev, model[1], target, 2, 2, eta=0.5)                   # no noise_seed: the step seeds stand in
    sched, sl = torch.tensor(SCHED4), eng.slot_len
    (c0, m0), (c1, m1) = _clip_canvas(eng, 3, 4), _clip_canvas(eng, 3, 5)
    kw = dict(step_seeds=[3, 4], init_canvases=[c0, c1], masks=[m0, m1], guide_seeds=[1, 2])
    a = A.fifo_denoise_clips(eng, pcs, hop, sched, 3, [31, 77], **kw)
    assert torch.isfinite(a).all() and not torch.equal(a[0], a[1])
    # a held region (mask 1) leaves the queue equal to its own clip's canvas bit for bit
    for k, c in enumerate((c0, c1)):
        assert torch.equal(a[k][:, sl:2 * sl], c[:, sl:2 * sl]) and not torch.equal(a[k][:, :sl], c[:, :sl])
    # the neighbour's prompt, seed, step seed and canvas do not reach clip 0
    b = A.fifo_denoise_clips(eng, [pcs[0], torch.flip(pcs[1], (1,)) * 0.5], hop, sched, 3, [31, 99], step_seeds=[3, 5],
                             init_canvases=[c0, c1 * 0.5], masks=[m0, m1], guide_seeds=[1, 7])
    assert torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1])
    # different step seeds with equal noise seeds and prompts give different clips; equal ones give equal clips
    d = A.fifo_denoise_clips(eng, [pcs[0], pcs[0]], hop, sched, 3, [31, 31], step_seeds=[3, 4])
    e = A.fifo_denoise_clips(eng, [pcs[0], pcs[0]], hop, sched, 3, [31, 31], step_seeds=[3, 3])
    assert not torch.equal(d[0], d[1]) and torch.equal(e[0], e[1]) and torch.equal(d[0], e[0])
    # without step seeds the eta > 0 engine is refused as before
    with pytest.raises(ValueError, match=r"eta == 0 \(the engine has eta = 0\.5\).*same step normals"):
        A.fifo_denoise_clips(eng, pcs, hop, sched, 3, [31, 77])


def test_step_seeds_on_an_eta_zero_engine_change_nothing(dev, model):
    import multimodal_diffusion_amd as A
    eng, pcs, hop = _setup(dev, model[1], "video", 2, 2)
    sched = torch.tensor(SCHED4)
    assert torch.equal(A.fifo_denoise_clips(eng, pcs, hop, sched, 3, [31, 77], step_seeds=[3, 4]),
                       A.fifo_denoise_clips(eng, pcs, hop, sched, 3, [31, 77]))


# ------------------------------------------------------------------------------------------------- 7. the pipeline
STREAM_ONE_SECOND = {"window_seconds": 1.0, "hop_seconds": 0.5, "crossfade_seconds": 0.25}


def test_pipeline_with_two_prompt_clips_at_eta_above_zero(dev, model):
    from multimodal_diffusion_amd import stream_infer as S
    vae, codec, cfg = pipeline(dev, seed=8, clip_seconds=1.0, sampler_steps=4, streaming=STREAM_ONE_SECOND, sampling={"ddim_eta": 0.5})
    wavs = [audio_prompt(36000)["prompt_audio"], audio_prompt(36000)["prompt_audio"][::-1].copy()]
    kw = dict(components(model[1], vae, codec, dev), cfg=cfg, prompt_modality="audio", prompt_video=None, sampler="fifo")
    res = S.stream_generate(prompt_audio=wavs, seed=[31, 31], noise_seed=[3, 4], **kw)
    single = S.stream_generate(prompt_audio=wavs[0], seed=31, noise_seed=3, **kw)
    assert isinstance(res, list) and len(res) == 2
    for r in res:
        assert r["video"].shape == single["video"].shape and r["video"].dtype == single["video"].dtype
        assert np.isfinite(r["video"].astype(np.float64)).all()
    assert not np.array_equal(res[0]["video"], res[1]["video"])
    with pytest.raises(ValueError, match=r"needs sampling.ddim_eta == 0 \(got 0\.5\)"):
        S.stream_generate(prompt_audio=wavs, seed=[31, 31], noise_seed=3, **kw)


# ------------------------------------------------------------------------------------------------- 8. AVD_EINVAL before the launch
@pytest.mark.parametrize("geom", [GEOMS[0], GEOMS[2]], ids=["video", "audio"])
def test_refusals_before_the_launch(dev, geom):
    L, Fn = _fn()
    K, B = geom[3], geom[1][0]
    _, sl, S, _, _ = _dims(geom)
    z, eps2, hist = _inputs(geom, dev)
    tn, tp, tl = _tables(B, S, dev)
    known, masks = _canvases(geom, dev)
    key = Fn.slot_key(0, 0, S, None, dev)
    guide = Fn.clip_guide(known[0], masks[0], 0, 0, S, None, tuple(z.shape))
    seeds = Fn.queue_seeds(SEEDS[:K], K, dev)

    def call(cq, eta=0.5, g=guide):
        return _run(dev, geom, z, eps2, tn, tp, None, None, eta, key, g, cq)

    call(L.ClipQueues(K, seeds.data_ptr(), seeds.data_ptr()))                     # the good call
    with pytest.raises(ValueError, match="queues must divide the batch"):
        call(L.ClipQueues(B - 1, seeds.data_ptr(), seeds.data_ptr()))
    with pytest.raises(ValueError, match="queues must divide the batch"):
        call(L.ClipQueues(0, seeds.data_ptr(), seeds.data_ptr()))
    with pytest.raises(ValueError, match="needs step_seeds"):
        call(L.ClipQueues(K, None, seeds.data_ptr()))
    call(L.ClipQueues(K, None, seeds.data_ptr()), eta=0.0)                        # not read at eta == 0: may be null
    with pytest.raises(ValueError, match="needs guide_seeds"):
        call(L.ClipQueues(K, seeds.data_ptr(), None))
    call(L.ClipQueues(K, seeds.data_ptr(), None), g=None)                         # not read without a guide
    with pytest.raises(ValueError, match="8-byte aligned"):
        call(L.ClipQueues(K, seeds.data_ptr() + 4, seeds.data_ptr()))
    # the canvases must not overlap z_out: canvas 0 starts 16 floats before z_out's end
    video = geom[0] == "video"
    out = torch.empty(known.numel() + z.numel(), device=dev)
    bad = Fn.clip_guide(known[0], None, 0, 0, S, None, tuple(z.shape))
    bad.known = out.data_ptr() + 4 * (z.numel() - 16)
    ab = ABAR.to(dev, torch.float32)
    name = "avd_cfg_unpatch_ddim" if video else "avd_cfg_untoken_ddim_audio"
    cq = L.ClipQueues(K, seeds.data_ptr(), seeds.data_ptr())
    dims = (B,) + tuple(geom[1][1:]) + tuple(geom[2])
    with pytest.raises(ValueError, match="known / mask must not overlap"):
        L.check(getattr(L.lib(), name + "_slots_clips_f32")(eps2.data_ptr(), z.data_ptr(), None, tn.data_ptr(), tp.data_ptr(), ab.data_ptr(),
                                                            T_TRAIN, GS, 0.5, C.byref(key), C.byref(bad), C.byref(cq), S, None,
                                                            out.data_ptr(), *dims, None, L.stream_ptr(dev)))
    # one canvas would pass where the K together do not: canvas 0 ends before z_out, canvas K - 1 does not
    front = torch.empty(known.numel() + z.numel(), device=dev)
    bad.known = front.data_ptr()
    zo = front[known[0].numel() + 16:]
    assert K > 1
    with pytest.raises(ValueError, match="known / mask must not overlap"):
        L.check(getattr(L.lib(), name + "_slots_clips_f32")(eps2.data_ptr(), z.data_ptr(), None, tn.data_ptr(), tp.data_ptr(), ab.data_ptr(),
                                                            T_TRAIN, GS, 0.5, C.byref(key), C.byref(bad), C.byref(cq), S, None,
                                                            zo.data_ptr(), *dims, None, L.stream_ptr(dev)))
    # the stand-alone passes take the same checks
    with pytest.raises(ValueError, match="queues must divide the batch"):
        Fn.slot_noise_clips(SEEDS[:K] + [1] * (B - 1 - K), tn, geom[1], sl)
    with pytest.raises(ValueError, match="null clip queues"):
        L.check(L.lib().avd_slot_noise_clips_f32(C.byref(key), None, tn.data_ptr(), z.data_ptr(), B, geom[1][1], geom[1][2], S, sl,
                                                 int(np.prod(geom[1][3:])), L.stream_ptr(dev)))
