"""The null CFG half without its duplicate prompt rows (avd_cfg_dedup_set, include/avdiff_hip.h): with the route on, the stacked
one-stream step in the audio -> video direction carries one prompt row per null sample instead of Np and copies its k / v into the
other key slots.  Everything here is an equality: route on and route off give the same bits, in the step's latent and in eps_tokens.
The models are the `_kit` ones at d = 512 with "s3_min_rows" lowered, so that these few hundred rows take the split-operand path the
route lives on.  The video -> audio direction stays on the full layout (not built), so it has no cases here."""
from contextlib import contextmanager

import pytest
import torch

from _kit import ABAR, dev, engine, modules, ts, video_case  # noqa: F401  (dev is a fixture)
from _tune import tuned
from conftest import rel_err
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu

GS = 3.5
TOL = 1e-4          # the parity tolerance of test_gpu_parity.py
REPL = "qkv3_replicate_kernel"


@contextmanager
def dedup(on):
    from multimodal_diffusion_amd import _lib as L
    prev = L.lib().avd_cfg_dedup_set(1 if on else 0)
    try:
        yield
    finally:
        L.lib().avd_cfg_dedup_set(prev)


@pytest.fixture(scope="module")
def model3(dev):
    """(ws, modules) of a 3-layer model: a middle block sees a shared prompt row that is no longer the zero row"""
    ws = R.synth_weights(seed=0, n_layers=3)
    return ws, modules(dev, ws, 3)


@pytest.fixture(autouse=True)
def split_path():
    with tuned(s3_min_rows=0):
        yield


def prompt(dev, B, n_prompt, seed=5):
    """an audio prompt latent of n_prompt tokens (chunk 4, stride 4)"""
    return torch.randn(B, 8, 4 * n_prompt, generator=torch.Generator().manual_seed(seed)).to(dev)


def replications(eng, z, tn, tp):
    """launches of the replication kernel in one step: the evidence of which route ran"""
    from multimodal_diffusion_amd import _lib as L
    L.prof_enable(True)
    try:
        eng.step(z, tn, tp)
        torch.cuda.synchronize()
    finally:
        L.prof_enable(False)
    return L.prof_report().get(REPL, (0, 0.0, 0.0))[0]


def both_routes(eng, z, tn, tp):
    """((latent, eps_tokens) with the route off, the same with it on)"""
    res = []
    for on in (False, True):
        with dedup(on):
            out = eng.step(z, tn, tp)
            res.append((out.clone(), eng.eps_tokens()))
    return res


def assert_equal_routes(eng, z, tn, tp):
    (z0, e0), (z1, e1) = both_routes(eng, z, tn, tp)
    assert torch.isfinite(z0).all() and torch.isfinite(e0).all()
    assert torch.equal(e1, e0), float((e1 - e0).abs().max())
    assert torch.equal(z1, z0), float((z1 - z0).abs().max())


def times(dev, B):
    return ts([981, 402, 17][:B], dev), ts([961, 382, -1][:B], dev)


# (2, 32): N = 74, N1 = 65, M0 = 148 — the segment boundary lies inside a 32-row tile and a 128-row image tile, the null queries
# cross the 64 mark; (3, 32): odd sample count; (2, 28): Nt = 56, qkv3_npad(N1) = 64 < qkv3_npad(N) = 128
@pytest.mark.parametrize("B,W", [(2, 32), (3, 32), (2, 28)])
def test_three_layer_step_is_bit_identical(dev, model3, B, W):
    z, za, npr = video_case(dev, B=B, W=W)
    eng = engine(model3[1], "video", tuple(z.shape), npr, guidance=GS, matmul="bf16x3")
    eng.set_prompt(za)
    tn, tp = times(dev, B)
    assert_equal_routes(eng, z, tn, tp)
    with dedup(True):
        assert replications(eng, z, tn, tp) == 3          # one per block: the route ran
    with dedup(False):
        assert replications(eng, z, tn, tp) == 0


def test_long_prompt_crosses_a_key_tile(dev, model3):
    """70 prompt tokens: the replicated slots 65 .. 133 cross the 64-key tile boundary at slot 128"""
    z, _, _ = video_case(dev, B=2, W=32)
    eng = engine(model3[1], "video", tuple(z.shape), 70, guidance=GS, matmul="bf16x3")
    eng.set_prompt(prompt(dev, 2, 70))
    assert_equal_routes(eng, z, *times(dev, 2))


@pytest.mark.parametrize("n_prompt,launches", [(1, 0), (2, 3)])
def test_shortest_prompts(dev, model3, n_prompt, launches):
    """one prompt token has no duplicate: the full route; two is the smallest real case"""
    z, _, _ = video_case(dev, B=2, W=32)
    eng = engine(model3[1], "video", tuple(z.shape), n_prompt, guidance=GS, matmul="bf16x3")
    eng.set_prompt(prompt(dev, 2, n_prompt))
    tn, tp = times(dev, 2)
    assert_equal_routes(eng, z, tn, tp)
    with dedup(True):
        assert replications(eng, z, tn, tp) == launches


@pytest.mark.parametrize("kw", [dict(), dict(solver="dpmpp_2m"), dict(guidance=[2.0, 5.0])], ids=["ddim", "dpmpp_2m", "per_sample_guidance"])
def test_trajectory_eager_and_graph(dev, model3, kw):
    """four steps driven by begin / advance, eager and as two replays of a captured pair, route on against route off"""
    z, za, npr = video_case(dev, B=2, W=32)
    sched = R.sampling_schedule(1000, 4)
    eng = engine(model3[1], "video", tuple(z.shape), npr, **dict(dict(guidance=GS, matmul="bf16x3"), **kw))
    eng.set_prompt(za)
    res = {}
    for on in (False, True):
        with dedup(on):
            eng.begin(sched)
            a, b = z.clone(), torch.empty_like(z)
            for _ in range(2):
                eng.advance(a, b)
                eng.advance(b, a)
            res[on, "eager"] = a.clone(), eng.eps_tokens()
            eng.begin(sched)
            a.copy_(z)
            pair = eng.capture_pair(a, b)
            pair.replay()
            pair.replay()
            res[on, "graph"] = a.clone(), eng.eps_tokens()
    z0, e0 = res[False, "eager"]
    assert torch.isfinite(z0).all()
    for k, (zk, ek) in res.items():
        assert torch.equal(zk, z0) and torch.equal(ek, e0), k


def test_strict_mode(dev, model3):
    """nine terms: the route is open to them, but the last block's residual row map exists on the six-term kernels only, so the step
    runs the full layout for now — equal either way"""
    z, za, npr = video_case(dev, B=2, W=32)
    eng = engine(model3[1], "video", tuple(z.shape), npr, guidance=GS, matmul="bf16x3_strict")
    eng.set_prompt(za)
    tn, tp = times(dev, 2)
    assert_equal_routes(eng, z, tn, tp)
    with dedup(True):
        assert replications(eng, z, tn, tp) in (0, 3)


@pytest.mark.parametrize("kw", [dict(matmul="f16x2"), dict(matmul="f32"), dict(matmul="bf16x3", split_streams=True)],
                         ids=["f16x2", "f32", "split_streams"])
def test_other_modes_fall_back(dev, model3, kw):
    """the switch is accepted and changes nothing: these steps run the full layout"""
    z, za, npr = video_case(dev, B=2, W=32)
    eng = engine(model3[1], "video", tuple(z.shape), npr, guidance=GS, **kw)
    eng.set_prompt(za)
    tn, tp = times(dev, 2)
    assert_equal_routes(eng, z, tn, tp)
    with dedup(True):
        assert replications(eng, z, tn, tp) == 0


def test_step_against_cpu_oracle(dev, model3):
    """the route's step is still the reference's step"""
    ws, mods = model3
    z, za, npr = video_case(dev, B=2, W=32)
    tn, tp = times(dev, 2)
    ref, ref_eps = R.denoise_step_a2v(z.cpu(), za.cpu(), tn.cpu(), tp.cpu(), ABAR, adapt_v=ws["adapt_v"], adapt_a=ws["adapt_a"],
                                      core=ws["core"], head=ws["head"], n_layers=3, n_heads=8, guidance=GS, return_eps=True)
    eng = engine(mods, "video", tuple(z.shape), npr, guidance=GS, matmul="bf16x3")
    eng.set_prompt(za)
    with dedup(True):
        out = eng.step(z, tn, tp)
        e2 = eng.eps_tokens()
    B = z.shape[0]
    e1, e0 = rel_err(out.cpu(), ref), rel_err((e2[B:] + GS * (e2[:B] - e2[B:])).cpu(), ref_eps)
    print(f"route on against the CPU oracle: latent {e1:.3e}, guided eps {e0:.3e}")
    assert e1 < TOL and e0 < TOL
