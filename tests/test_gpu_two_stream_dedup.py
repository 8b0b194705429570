"""The short null layout under two streams (DenoiseEngine(split_streams="short"), avd_step_desc.split_streams == 2): the cond half runs
as B samples of N rows on the caller's stream, the null half as an all-short batch of Nt + 1 rows per sample on the second stream,
the null chain trailing the cond chain by the "cfg_offset" tune key's launches.  Everything here is an equality of bits between
three forms of the same bf16x3 step — two streams with the short layout, one stream with it, two streams (split_streams=True) with
the route switched off (avd_cfg_dedup_set(0): the full layout in both chains) — for one step, for a four-step trajectory, and for the trajectory replayed
from a captured pair at every "cfg_offset".  The models are the `_kit` ones (d = 512, 2 layers) with "s3_min_rows" lowered so that
these few hundred rows take the split-operand path the route lives on."""
from contextlib import contextmanager

import pytest
import torch

from _kit import dev, engine, model, ts  # noqa: F401  (dev, model are fixtures)
from _tune import tuned
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu

GS = 3.5
REPL = "qkv3_replicate_kernel"
OFFSET_DEFAULT = 0          # g_cfg_offset in csrc/composite.hip
# (B, W, Np): the video latent is [B, 8, 4, 16, W], Nt = 2 W target tokens, and the audio prompt has Np tokens.
#   W = 48, Np = 2: Nt = 96, N = 98, the null samples keep 97 rows — the 32-row wave tile that starts at row 96 and the 64-key tile that
#   starts at key 64 both end inside the prompt rows; the smallest prompt the route takes
#   W = 32, Np = 37: Nt = 64, N = 101 — the flagship's prompt length; the replicated key slots 65 .. 100 lie in the second key tile
#   B = 3: a ragged stacked batch — an odd sample count per half, 294 / 303 cond rows (more than one 256-row block), 291 / 195 null rows
CASES = [(2, 48, 2), (3, 48, 2), (2, 32, 37), (3, 32, 37)]
IDS = [f"B{b}-Nt{2 * w}-Np{n}" for b, w, n in CASES]
FORMS = {"two_short": ("short", True), "one_short": (False, True), "two_full": (True, False)}


@contextmanager
def dedup(on):
    from multimodal_diffusion_amd import _lib as L
    prev = L.lib().avd_cfg_dedup_set(1 if on else 0)
    try:
        yield
    finally:
        L.lib().avd_cfg_dedup_set(prev)


@contextmanager
def cfg_offset(k):
    from multimodal_diffusion_amd import _lib as L
    L.check(L.lib().avd_tune_set(b"cfg_offset", k))
    try:
        yield
    finally:
        L.check(L.lib().avd_tune_set(b"cfg_offset", OFFSET_DEFAULT))


@pytest.fixture(autouse=True)
def split_path():
    with tuned(s3_min_rows=0):
        yield


def inputs(dev, B, W, n_prompt):
    g = torch.Generator().manual_seed(1000 * B + W + n_prompt)
    z = torch.randn(B, 8, 4, 16, W, generator=g).to(dev)
    za = torch.randn(B, 8, 4 * n_prompt, generator=g).to(dev)
    tn, tp = ts([981, 402, 17][:B], dev), ts([961, 382, -1][:B], dev)
    return z, za, tn, tp


def make(mods, form, z, za, n_prompt):
    split, _ = FORMS[form]
    eng = engine(mods, "video", tuple(z.shape), n_prompt, guidance=GS, matmul="bf16x3", split_streams=split)
    eng.set_prompt(za)
    return eng


def eager(eng, z, tn, tp, sched):
    """(one step's latent, its eps tokens, the latent after four steps driven by begin / advance, its last eps tokens)"""
    out = eng.step(z, tn, tp).clone()
    eps = eng.eps_tokens().clone()
    eng.begin(sched)
    a, b = z.clone(), torch.empty_like(z)
    for _ in range(2):
        eng.advance(a, b)
        eng.advance(b, a)
    return out, eps, a.clone(), eng.eps_tokens().clone()


def replayed(eng, z, sched):
    eng.begin(sched)
    a, b = z.clone(), torch.empty_like(z)
    pair = eng.capture_pair(a, b)
    pair.replay()
    pair.replay()
    return a.clone(), eng.eps_tokens().clone()


@pytest.fixture(scope="module")
def one_stream(dev, model):
    """the one-stream short-layout results of each case, computed once: (step latent, step eps, trajectory latent, trajectory eps)"""
    cache = {}

    def get(case):
        if case not in cache:
            z, za, tn, tp = inputs(dev, *case)
            with dedup(True):          # (called from inside a test: "s3_min_rows" is lowered)
                cache[case] = eager(make(model[1], "one_short", z, za, case[2]), z, tn, tp, R.sampling_schedule(1000, 4))
            assert all(torch.isfinite(t).all() for t in cache[case])
        return cache[case]
    return get


def same(got, want, what):
    for name, g, w in zip(("step latent", "step eps", "trajectory latent", "trajectory eps"), got, want):
        d = (g - w).abs()
        assert torch.equal(g, w), f"{what}, {name}: max |diff| {float(d.max()):.3e} in {int((d > 0).sum())} elements"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_step_and_trajectory_are_bit_identical(dev, model, one_stream, case):
    z, za, tn, tp = inputs(dev, *case)
    sched = R.sampling_schedule(1000, 4)
    ref = one_stream(case)
    for form in ("two_short", "two_full"):
        with dedup(FORMS[form][1]):
            eng = make(model[1], form, z, za, case[2])
            same(eager(eng, z, tn, tp, sched), ref, form)
            if form == "two_full":          # (the offset belongs to the short form: its replays are the next test)
                same(replayed(eng, z, sched), ref[2:], "two_full replayed")


@pytest.mark.parametrize("k", [0, 1, 2, 3])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_captured_pair_replays_at_every_offset(dev, model, one_stream, case, k):
    """the two-stream short form at each offset: the step captured with fork / lead / join inside one capture and replayed twice (the
    four-step trajectory), and the eager step and trajectory"""
    z, za, tn, tp = inputs(dev, *case)
    sched = R.sampling_schedule(1000, 4)
    ref = one_stream(case)
    with cfg_offset(k):
        with dedup(True):
            eng = make(model[1], "two_short", z, za, case[2])
            same(replayed(eng, z, sched), ref[2:], f"replayed, cfg_offset {k}")
            same(eager(eng, z, tn, tp, sched), ref, f"eager, cfg_offset {k}")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kernels_of_the_two_stream_short_form(dev, model, case):
    """one replication launch per block per step, and the GEMM / attention kernels of the one-stream short form: both chains plan
    their launches for the stacked 2B x N batch"""
    from multimodal_diffusion_amd import _lib as L
    z, za, tn, tp = inputs(dev, *case)
    tags, counts = {}, {}
    for form in ("two_short", "one_short", "two_full"):
        with dedup(FORMS[form][1]):
            eng = make(model[1], form, z, za, case[2])
            eng.step(z, tn, tp)
            L.prof_enable(True)
            try:
                eng.step(z, tn, tp)
                torch.cuda.synchronize()
            finally:
                L.prof_enable(False)
        rep = L.prof_report()
        counts[form] = rep.get(REPL, (0,))[0]
        tags[form] = {t for t, v in rep.items() if v[0] > 0 and t.startswith(("gemm_bf16x3", "attn_bf16x3"))}
    assert counts == {"two_short": 2, "one_short": 2, "two_full": 0}, counts
    assert any(t.startswith("gemm_bf16x3") for t in tags["one_short"]) and any(t.startswith("attn_bf16x3") for t in tags["one_short"])
    assert tags["two_short"] == tags["one_short"], (tags["one_short"], tags["two_short"])


def test_split_streams_true_keeps_the_full_layout(dev, model):
    """split_streams=True is the two-chain step as it was: the full layout whatever the route's switch says"""
    from multimodal_diffusion_amd import _lib as L
    z, za, tn, tp = inputs(dev, *CASES[0])
    eng = engine(model[1], "video", tuple(z.shape), CASES[0][2], guidance=GS, matmul="bf16x3", split_streams=True)
    eng.set_prompt(za)
    with dedup(True):
        L.prof_enable(True)
        try:
            eng.step(z, tn, tp)
            torch.cuda.synchronize()
        finally:
            L.prof_enable(False)
    assert L.prof_report().get(REPL, (0,))[0] == 0
    with pytest.raises(ValueError):
        engine(model[1], "video", tuple(z.shape), CASES[0][2], guidance=GS, matmul="bf16x3", split_streams="long")


def test_default_and_where_the_layout_does_not_apply(dev, model):
    """split_streams=None: bf16x3 takes the two chains with the short layout from 24,321 stacked rows where the layout applies;
    "short" where it does not apply (video -> audio) is the one-stream step"""
    from _kit import audio_case
    shape = (29, 8, 12, 32, 32)          # 2 x 29 x 421 = 24,418 stacked rows: the first batch at or above 24,321
    for kw, want in ((dict(matmul="bf16x3"), (True, True)), (dict(matmul="bf16x3", attn="fp8"), (False, False)),
                     (dict(matmul="f32"), (False, False)),
                     (dict(matmul="f16x2"), (True, False)), (dict(matmul="bf16x3", split_streams=False), (False, False))):
        eng = engine(model[1], "video", shape, 37, guidance=GS, **kw)
        assert (eng._split_streams, eng._split_short) == want, kw
    small = engine(model[1], "video", (28, 8, 12, 32, 32), 37, guidance=GS, matmul="bf16x3")          # 23,576 stacked rows
    assert not small._split_streams
    z, zv, npr = audio_case(dev, B=2)
    tn, tp = ts([981, 402], dev), ts([961, 382], dev)
    outs = []
    for split in ("short", False):
        eng = engine(model[1], "audio", tuple(z.shape), npr, guidance=GS, matmul="bf16x3", split_streams=split)
        assert not eng._split_streams and eng.desc.split_streams == 0
        eng.set_prompt(zv)
        outs.append(eng.step(z, tn, tp).clone())
    assert torch.equal(outs[0], outs[1])


def test_slot_form_takes_the_two_chains(dev, model):
    """uniform slot tables through step_slots: the plain step's bits, on the two chains with the short layout"""
    from multimodal_diffusion_amd import _lib as L
    z, za, tn, tp = inputs(dev, *CASES[2])
    with dedup(True):
        eng = make(model[1], "two_short", z, za, CASES[2][2])
        ref = eng.step(z, tn, tp).clone()
        L.prof_enable(True)
        try:
            out = eng.step_slots(z, tn[:, None].expand(2, eng.slots).contiguous(), tp[:, None].expand(2, eng.slots).contiguous())
            torch.cuda.synchronize()
        finally:
            L.prof_enable(False)
    assert L.prof_report().get(REPL, (0,))[0] == 2
    assert torch.equal(out, ref)
