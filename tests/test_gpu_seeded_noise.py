"""The seeded DDIM noise stream on the MI355X (include/avdiff_hip.h, avd_noise_key): avd_gaussian_noise_f32 against the numpy
reference and normal statistics, the fused seeded step against the unseeded step fed the same noise explicitly (both DDIM kernel
forms, the audio target, split streams), graph replay against eager launches, batch / offset invariance, eta > 0 trajectories
against the CPU oracle, the unchanged behaviour without a seed, and a sharded stream_generate against the single-process run."""
import json
import os
import subprocess
import sys
from functools import partial
from pathlib import Path

import numpy as np
import pytest
import torch

from _kit import ABAR, audio_case, dev, engine, free_port, model, video_case  # noqa: F401  (dev / model are fixtures)
from _noise_ref import normals
from _tune import cfg_rows  # noqa: F401  (fixture)
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SEED = 0xDEADBEEF12345678           # both key words non-zero
ETA = 0.5
_engine = partial(engine, guidance=3.0)        # engine(mods, target, shape, n_prompt, **kw) at this file's guidance


# ------------------------------------------------------------------------------------------------- the generator
def test_generator_matches_reference(dev):
    from multimodal_diffusion_amd import functional as Fn
    per = 524_291                                             # not a multiple of 4
    for seed, off, tn in ((SEED, 0, [999, 980, 500, 17, 0, 1, 999, 3]), (7, 1000, [5, 5, 5, 5, 5, 5, 5, 5]),
                          (2 ** 64 - 1, 2 ** 32 - 8, [-1, 2 ** 40 + 3, 20, 21, 22, 23, 24, 25])):
        t = torch.tensor(tn, dtype=torch.long, device=dev)
        got = Fn.gaussian_noise(seed, off, t, (8, per)).cpu().numpy().astype(np.float64)
        ref = normals(seed, off, tn, per)
        assert got.shape == ref.shape and got.size >= 2 ** 22
        err = np.abs(got - ref).max()
        assert err < 1e-5, (seed, off, err)


def test_generator_statistics(dev):
    from multimodal_diffusion_amd import functional as Fn
    B, per = 16, 1 << 18
    x = Fn.gaussian_noise(SEED, 0, torch.full((B,), 731, dtype=torch.long, device=dev), (B, per)).double()
    n = x.numel()
    assert n >= 2 ** 22
    mean, var = float(x.mean()), float(x.var())
    kurt = float(((x - mean) ** 4).mean() / var ** 2)
    assert abs(mean) < 2.5e-3 and abs(var - 1) < 3.5e-3 and abs(kurt - 3) < 0.03, (mean, var, kurt)
    xs = torch.sort(x.flatten())[0]
    cdf = torch.special.ndtr(xs)
    i = torch.arange(1, n + 1, device=dev, dtype=torch.float64)
    D = float(torch.maximum(i / n - cdf, cdf - (i - 1) / n).max())
    assert D < 1.95 / n ** 0.5, D

    def corr(a, b):
        a, b = a.flatten() - a.mean(), b.flatten() - b.mean()
        return float((a * b).sum() / (a.norm() * b.norm()))
    lim = lambda m: 5 / m ** 0.5                                          # noqa: E731
    assert abs(corr(x[:, :-1], x[:, 1:])) < lim(B * (per - 1))           # neighbouring elements
    assert abs(corr(x[:-1], x[1:])) < lim((B - 1) * per)                 # neighbouring sample indices, same t
    y = Fn.gaussian_noise(SEED, 0, torch.full((B,), 732, dtype=torch.long, device=dev), (B, per)).double()
    assert abs(corr(x, y)) < lim(n)                                      # neighbouring timesteps, same samples


def test_stream_batch_and_offset_invariance(dev, model):
    from multimodal_diffusion_amd import functional as Fn
    tn = torch.tensor([999, 500, 500, 3], dtype=torch.long, device=dev)
    shape = (4, 8, 4, 16, 32)
    whole = Fn.gaussian_noise(SEED, 0, tn, shape)
    for k in range(4):
        assert torch.equal(Fn.gaussian_noise(SEED, k, tn[k:k + 1], (1,) + shape[1:]), whole[k:k + 1])
    # a seeded engine at sample_offset = k uses row k of the stream
    z, za, npr = video_case(dev, B=1)
    tp = tn - 20
    k = 2
    seeded = _engine(model[1], "video", tuple(z.shape), npr, eta=ETA, noise_seed=SEED, sample_offset=k)
    plain = _engine(model[1], "video", tuple(z.shape), npr, eta=ETA)
    for e in (seeded, plain):
        e.set_prompt(za)
    a = seeded.step(z, tn[k:k + 1], tp[k:k + 1])
    b = plain.step(z, tn[k:k + 1], tp[k:k + 1], noise=whole[k:k + 1])
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------- fused = explicit
@pytest.mark.parametrize("rows", [1, 0])
def test_fused_step_equals_explicit_noise_video(dev, model, cfg_rows, rows):
    from multimodal_diffusion_amd import functional as Fn
    cfg_rows(rows)
    z, za, npr = video_case(dev, B=3)
    tn = torch.tensor([981, 402, 40], dtype=torch.long, device=dev)
    tp = torch.tensor([961, 382, -1], dtype=torch.long, device=dev)
    seeded = _engine(model[1], "video", tuple(z.shape), npr, eta=ETA, noise_seed=SEED, sample_offset=5)
    plain = _engine(model[1], "video", tuple(z.shape), npr, eta=ETA)
    for e in (seeded, plain):
        e.set_prompt(za)
    a = seeded.step(z, tn, tp)
    b = plain.step(z, tn, tp, noise=Fn.gaussian_noise(SEED, 5, tn, tuple(z.shape)))
    assert torch.equal(a, b)
    c = plain.step(z, tn, tp, noise=Fn.gaussian_noise(SEED + 1, 5, tn, tuple(z.shape)))
    assert not torch.equal(a, c)                              # the noise term is live


def test_fused_step_equals_explicit_noise_audio(dev, model):
    from multimodal_diffusion_amd import functional as Fn
    z, zv, npr = audio_case(dev, B=3)
    tn = torch.tensor([981, 402, 40], dtype=torch.long, device=dev)
    tp = torch.tensor([961, 382, -1], dtype=torch.long, device=dev)
    seeded = _engine(model[1], "audio", tuple(z.shape), npr, eta=ETA, noise_seed=SEED, sample_offset=11)
    plain = _engine(model[1], "audio", tuple(z.shape), npr, eta=ETA)
    for e in (seeded, plain):
        e.set_prompt(zv)
    a = seeded.step(z, tn, tp)
    assert torch.equal(a, plain.step(z, tn, tp, noise=Fn.gaussian_noise(SEED, 11, tn, tuple(z.shape))))


def test_fused_step_equals_explicit_noise_split_streams_f16x2(dev, model):
    from multimodal_diffusion_amd import functional as Fn
    z, za, npr = video_case(dev, B=2)
    tn = torch.tensor([700, 300], dtype=torch.long, device=dev)
    tp = torch.tensor([680, 280], dtype=torch.long, device=dev)
    kw = dict(eta=ETA, matmul="f16x2", split_streams=True)
    seeded = _engine(model[1], "video", tuple(z.shape), npr, noise_seed=SEED, **kw)
    plain = _engine(model[1], "video", tuple(z.shape), npr, **kw)
    for e in (seeded, plain):
        e.set_prompt(za)
    assert torch.equal(seeded.step(z, tn, tp), plain.step(z, tn, tp, noise=Fn.gaussian_noise(SEED, 0, tn, tuple(z.shape))))


# ------------------------------------------------------------------------------------------------- graph = eager
@pytest.mark.parametrize("n_steps", [5, 6])
def test_seeded_graph_equals_eager(dev, model, n_steps):
    from multimodal_diffusion_amd import functional as Fn
    z, za, npr = video_case(dev, B=2)
    sched = torch.linspace(999, 0, n_steps + 1).round().long()
    sched[-1] = -1
    seeded = _engine(model[1], "video", tuple(z.shape), npr, eta=ETA, noise_seed=SEED)
    seeded.set_prompt(za)
    zg = seeded.run(z, sched, graph=True)
    ze = seeded.run(z, sched, graph=False)
    assert torch.equal(zg, ze)
    assert torch.equal(seeded.run(z, sched), zg)             # graph=None takes the graph here (2B*N < 6,144 rows)
    # every step drew the noise of its own t_now: the unseeded engine fed the stream step by step lands on the same bits
    plain = _engine(model[1], "video", tuple(z.shape), npr, eta=ETA)
    plain.set_prompt(za)
    x = z.clone()
    for i in range(n_steps):
        tn = torch.full((2,), int(sched[i]), dtype=torch.long, device=dev)
        tp = torch.full((2,), int(sched[i + 1]), dtype=torch.long, device=dev)
        x = plain.step(x, tn, tp, noise=Fn.gaussian_noise(SEED, 0, tn, tuple(z.shape)))
    assert torch.equal(x, zg)
    n0 = Fn.gaussian_noise(SEED, 0, torch.full((2,), int(sched[0]), device=dev), tuple(z.shape))
    n1 = Fn.gaussian_noise(SEED, 0, torch.full((2,), int(sched[1]), device=dev), tuple(z.shape))
    assert not torch.equal(n0, n1)


# ------------------------------------------------------------------------------------------------- trajectory vs the oracle
@pytest.mark.parametrize("target", ["video", "audio"])
def test_seeded_trajectory_vs_oracle(dev, model, target):
    from multimodal_diffusion_amd import functional as Fn
    ws, _ = model
    n_steps = 8
    sched = R.sampling_schedule(1000, n_steps)
    if target == "video":
        z, zp, npr = video_case(dev, B=2, W=16)
    else:
        z, zp, npr = audio_case(dev, B=2)
    eng = _engine(model[1], target, tuple(z.shape), npr, eta=ETA, noise_seed=SEED, sample_offset=3)
    eng.set_prompt(zp)
    out = eng.run(z, sched).cpu().double()
    x, p = z.cpu(), zp.cpu()
    kw = dict(adapt_v=ws["adapt_v"], adapt_a=ws["adapt_a"], core=ws["core"], head=ws["head"], n_layers=2, n_heads=8, guidance=3.0,
              eta=0.0, return_eps=True)
    for i in range(len(sched) - 1):
        tn, tp = sched[i].repeat(2), sched[i + 1].repeat(2)
        if target == "video":
            _, eps_tok = R.denoise_step_a2v(x, p, tn, tp, ABAR, **kw)
            eps = R.tube_unpatch(eps_tok, *x.shape[1:], 2, 4, 4)
        else:
            _, eps_tok = R.denoise_step_v2a(x, p, tn, tp, ABAR, **kw)
            eps = R.audio_untokens(eps_tok, x.shape[1], 4, x.shape[2], 4)
        noise = Fn.gaussian_noise(SEED, 3, tn.to(dev), tuple(x.shape)).cpu()
        x = R.ddim_update(x, tn, tp, eps, ABAR, eta=ETA, noise=noise)
    ref = x.double()
    assert float((out - ref).norm() / ref.norm()) < 1e-3


# ------------------------------------------------------------------------------------------------- no behaviour change
def test_no_behaviour_change_without_eta_or_seed(dev, model):
    z, za, npr = video_case(dev, B=2)
    tn = torch.tensor([900, 100], dtype=torch.long, device=dev)
    tp = torch.tensor([880, 80], dtype=torch.long, device=dev)
    seeded0 = _engine(model[1], "video", tuple(z.shape), npr, eta=0.0, noise_seed=SEED)
    plain0 = _engine(model[1], "video", tuple(z.shape), npr, eta=0.0)
    for e in (seeded0, plain0):
        e.set_prompt(za)
    assert torch.equal(seeded0.step(z, tn, tp), plain0.step(z, tn, tp))
    unseeded = _engine(model[1], "video", tuple(z.shape), npr, eta=ETA)
    unseeded.set_prompt(za)
    unseeded.begin(torch.tensor([999, 500, -1]))
    with pytest.raises(NotImplementedError):
        unseeded.capture_pair(z.clone(), torch.empty_like(z))
    seeded = _engine(model[1], "video", tuple(z.shape), npr, eta=ETA, noise_seed=SEED)
    seeded.set_prompt(za)
    with pytest.raises(ValueError):
        seeded.step(z, tn, tp, noise=torch.randn_like(z))
    for bad in (dict(noise_seed=-1), dict(noise_seed=2 ** 64), dict(noise_seed=1, sample_offset=-1), dict(sample_offset=3)):
        with pytest.raises(ValueError):
            _engine(model[1], "video", tuple(z.shape), npr, eta=ETA, **bad)


# ------------------------------------------------------------------------------------------------- sharded = single process
@pytest.mark.gpu_first
def test_stream_generate_seeded_eta_sharded_two_ranks_share_device(tmp_path):
    """stream_generate(shard=True) with ddim_eta 0.5 and noise_seed, as two fresh ranks under torch.distributed.run (gloo, both on
    cuda:0): the stitched video (audio prompt) and waveform (video prompt) equal the single-process results bit for bit, and so does
    a single-process run with max_windows_per_batch=1 (tests/_stream_shard_seeded_worker.py).  This process never touches the device."""
    if torch.cuda.device_count() < 1:
        pytest.skip("needs a GPU")
    if torch.cuda.is_initialized():
        pytest.skip("this process already initialised the GPU: run this test first / alone (conftest orders it first)")
    out = tmp_path / "shard.json"
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", AVD_TEST_OUT=str(out))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), str(ROOT / "tests" / "_stream_shard_seeded_worker.py")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    d = json.loads(out.read_text())
    assert d["world"] == 2 and d["windows"] == 4 and d["audio_windows"] == 2, d
    assert d["video_sharded_equal"] and d["video_per_window_equal"], d
    assert d["audio_sharded_equal"] and d["audio_per_window_equal"], d
    assert d["eta_changes_result"], d
