"""GPU parity: every HIP kernel / composite, called through the C ABI, against the CPU oracle and the
reference-generated golden fixtures.  Tolerance: max|Δ| <= 1e-4 * max(1, max|ref|) per function and
per single step; chained trajectory: relative L2 <= 1e-3."""
import json
import math
import re

import numpy as np
import pytest
import torch

from _attn_kit import split3_decode as _split3_decode
from _kit import STREAM_HALF_SECOND, components, dev, engine, full, grp, modules, pipeline  # noqa: F401  (dev / full are fixtures)
from _tune import tune, tuned
from conftest import load_golden, rel_err, split_weights
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
TOL = 1e-4


def T(a):
    return torch.from_numpy(np.asarray(a))


def G(a, dev):
    return torch.as_tensor(np.asarray(a)).to(dev)


# ------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("M,N,K", [(1, 32, 32), (77, 64, 64), (130, 96, 128), (421, 1536, 512), (842, 512, 2048),
                                   (300, 256, 256), (1000, 32, 512), (64, 2048, 512), (5, 512, 36), (4000, 640, 512)])
@pytest.mark.parametrize("mode", ["plain", "gelu", "res"])
def test_gemm(dev, M, N, K, mode):
    from multimodal_diffusion_amd import functional as Fn, _lib as L
    g = torch.Generator().manual_seed(M * 7 + N + K)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    b = torch.randn(N, generator=g)
    r = torch.randn(M, N, generator=g)
    ref = R.linear(x.double(), w.double(), b.double())
    if mode == "gelu":
        ref = R.gelu_erf(ref)
    if mode == "res":
        ref = ref + r.double()
    y = Fn.linear(x.to(dev), w.to(dev), b.to(dev), act=L.ACT_GELU if mode == "gelu" else L.ACT_NONE,
                  residual=r.to(dev) if mode == "res" else None)
    assert rel_err(y.cpu(), ref) < 2e-5


def test_gemm_asymmetric_identity(dev):
    # A = I with an asymmetric W catches a transposed C write (MFMA layout check)
    from multimodal_diffusion_amd import functional as Fn
    n = 96
    w = torch.arange(n * n, dtype=torch.float32).view(n, n)
    y = Fn.linear(torch.eye(n).to(dev), w.to(dev))
    assert torch.equal(y.cpu(), w.t().contiguous())


@pytest.mark.parametrize("B,N,H", [(1, 13, 1), (2, 64, 2), (2, 70, 2), (1, 133, 8), (2, 421, 8), (1, 43, 8), (1, 257, 4)])
def test_attention(dev, B, N, H):
    from multimodal_diffusion_amd import functional as Fn
    g = torch.Generator().manual_seed(B * 1000 + N)
    d = 64 * H
    qkv = torch.randn(B, N, 3 * d, generator=g) * 1.5
    q, k, v = (qkv.double().view(B, N, 3, H, 64)[:, :, i].transpose(1, 2) for i in range(3))
    ref = (torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1) @ v).transpose(1, 2).reshape(B, N, d)
    y = Fn.attention(qkv.to(dev), H)
    assert rel_err(y.cpu(), ref) < 2e-5


def test_attention_spiky_scores(dev):
    # one key dominates late in the sequence: exercises the online-softmax rescale across tiles
    from multimodal_diffusion_amd import functional as Fn
    g = torch.Generator().manual_seed(5)
    B, N, H, d = 1, 200, 1, 64
    qkv = torch.randn(B, N, 3 * d, generator=g)
    qkv[0, 3, :64] *= 6.0
    qkv[0, 170, 64:128] = qkv[0, 3, :64] * 1.0          # key 170 aligned with query 3
    q, k, v = (qkv.double().view(B, N, 3, H, 64)[:, :, i].transpose(1, 2) for i in range(3))
    ref = (torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1) @ v).transpose(1, 2).reshape(B, N, d)
    assert rel_err(Fn.attention(qkv.to(dev), H).cpu(), ref) < 2e-5


def test_attention_n_query(dev):
    from multimodal_diffusion_amd import functional as Fn
    qkv = torch.randn(2, 100, 3 * 128, generator=torch.Generator().manual_seed(1)).to(dev)
    full = Fn.attention(qkv, 2)
    part = Fn.attention(qkv, 2, n_query=40)
    assert torch.equal(part[:, :40], full[:, :40])
    assert torch.count_nonzero(part[:, 40:]) == 0


def test_rmsnorm_golden(dev):
    from multimodal_diffusion_amd import RMSNorm
    g = load_golden("g4_rmsnorm.npz")
    n = RMSNorm(512).to(dev)
    n.load_state_dict({"scale": T(g["scale"])})
    y = n(G(g["x"], dev)).cpu()
    assert rel_err(y, g["y"]) < 1e-6
    assert torch.equal(y[2], torch.zeros(512))


@pytest.mark.parametrize("d", [64, 128, 512, 1024, 2048])
def test_rmsnorm_and_layernorm_widths(dev, d):
    from multimodal_diffusion_amd import functional as Fn, _lib as L
    g = torch.Generator().manual_seed(d)
    x = torch.randn(37, d, generator=g) * 3 + 0.5
    s = torch.randn(d, generator=g)
    b = torch.randn(d, generator=g)
    assert rel_err(Fn.rmsnorm(x.to(dev), s.to(dev)).cpu(), R.rmsnorm(x.double(), s.double())) < 1e-6
    ref = R.gelu_erf(R.layernorm(x.double(), s.double(), b.double()))
    assert rel_err(Fn.layernorm_act(x.to(dev), s.to(dev), b.to(dev), act=L.ACT_GELU).cpu(), ref) < 2e-6


def test_timestep_embedding_golden(dev):
    from multimodal_diffusion_amd import schedule_utils as su, functional as Fn
    g = load_golden("g2_temb.npz")
    t = G(g["t"], dev)
    for dim, key in ((256, "e256"), (64, "e64"), (7, "e7")):
        got = su.timestep_embedding(t, dim).cpu()
        # (1) tight: kernel cos/sin against fp64 cos/sin of the SAME fp32 angle t*f (f = the uploaded table)
        f = Fn.temb_freqs(dim, 10000, dev).cpu()
        ang = (T(g["t"]).float()[:, None] * f[None, :]).double()
        exact = torch.cat([ang.cos(), ang.sin()], 1)
        if dim % 2:
            exact = torch.nn.functional.pad(exact, (0, 1))
        assert rel_err(got, exact) < 1e-6, dim
        # (2) golden from the reference run in the build container.  f = exp(.) is evaluated by the HOST's vectorised
        # fp32 exp, which differs by 1 ulp between CPU generations; at t = 999 that moves the angle by
        # 999 * 2^-24 = 6e-5, so the reference itself is only reproducible to ~1.2e-4 across machines.
        assert rel_err(got, g[key]) < 1.2e-4, dim
    e0 = su.timestep_embedding(torch.zeros(3, dtype=torch.long, device=dev), 256).cpu()
    assert torch.equal(e0[:, :128], torch.ones(3, 128)) and torch.equal(e0[:, 128:], torch.zeros(3, 128))


def test_patch_unpatch_golden_and_roundtrip(dev):
    from multimodal_diffusion_amd import ops
    g = load_golden("g3_index.npz")
    for key in [k for k in g if k.startswith("patch/")]:
        C, Tt, H, W = map(int, key.split("/")[1].split("x"))
        z = torch.arange(C * Tt * H * W, dtype=torch.float32).view(1, C, Tt, H, W).to(dev)
        tok = ops.tube_patch_video(z, 2, 4, 4)
        assert np.array_equal(tok.cpu().numpy().astype(np.int32), g[key])
        assert torch.equal(ops.tube_unpatch_video(tok, C, Tt, H, W, 2, 4, 4), z)
    # the reference's own value-level test (tests/test_shapes.py:26-36)
    torch.manual_seed(0)
    z = torch.randn(2, 8, 12, 16, 16).to(dev)
    tok = ops.tube_patch_video(z, 2, 4, 4)
    assert tok.shape == (2, 96, 256)
    assert torch.allclose(z, ops.tube_unpatch_video(tok, C=8, T=12, H=16, W=16, t=2, h=4, w=4), atol=1e-6)
    with pytest.raises(AssertionError):
        ops.tube_patch_video(torch.zeros(1, 8, 3, 16, 16, device=dev), 2, 4, 4)
    with pytest.raises(AssertionError):
        ops.tube_unpatch_video(tok, C=8, T=12, H=16, W=16, t=2, h=4, w=8)


def test_audio_tokens_golden(dev):
    from multimodal_diffusion_amd import sampler as S, ops
    g = load_golden("g3_index.npz")
    za = torch.arange(2 * 8 * 150, dtype=torch.float32).view(2, 8, 150).to(dev)
    tok = S.latents_to_tokens_audio(za, 4, 4)
    assert np.array_equal(tok.cpu().numpy().astype(np.int32), g["audio_tok/150"])
    un = S.tokens_to_latents_audio(tok + 1.0, Ca=8, l_chunk=4, Fa=150, stride=4)
    assert np.array_equal(un.cpu().numpy().astype(np.int32), g["audio_untok/150"])
    assert np.array_equal(S.tokens_to_latents_audio(G(g["audio22/tok"], dev), 8, 4, 22, 4).cpu().numpy(), g["audio22/untok"])
    assert np.array_equal(S.latents_to_tokens_audio(G(g["audio22/z"], dev), 4, 2).cpu().numpy(), g["audio22s2/tok"])
    got = S.tokens_to_latents_audio(G(g["audio22s2/tok"], dev), 8, 4, 22, 2).cpu().numpy()
    assert np.allclose(got, g["audio22s2/untok"], atol=1e-6)
    # generic overlap_add_1d / chunk_1d shapes as in the reference's tests/test_shapes.py:38-49
    x = torch.randn(2, 8, 150, device=dev)
    win = ops.chunk_1d(x, length=4, stride=4)
    assert win.shape == (2, 8, 37, 4)
    y = ops.overlap_add_1d(win, stride=4, length=4)
    assert y.shape == (2, 8, 148) and torch.equal(y, x[..., :148])


def test_ddim_golden(dev):
    from multimodal_diffusion_amd import schedule_utils as su
    g = load_golden("g7_ddim.npz")
    y = su.ddim_step(G(g["x_t"], dev), G(g["t_now"], dev), G(g["t_prev"], dev), G(g["eps"], dev), T(g["abar"]))
    assert rel_err(y.cpu(), g["x_prev"]) < 1e-6
    # eta > 0 with caller-supplied noise vs oracle
    nz = torch.randn(5, 8, 2, 4, 4, generator=torch.Generator().manual_seed(3))
    y = su.ddim_step(G(g["x_t"], dev), G(g["t_now"], dev), G(g["t_prev"], dev), G(g["eps"], dev), T(g["abar"]), eta=0.7,
                     noise=nz.to(dev))
    ref = R.ddim_update(T(g["x_t"]), T(g["t_now"]), T(g["t_prev"]), T(g["eps"]), T(g["abar"]), eta=0.7, noise=nz)
    assert rel_err(y.cpu(), ref) < 1e-6


# ------------------------------------------------------------------------------------------------- modules
def _small_modules(dev, W, meta):
    import multimodal_diffusion_amd as A
    core = A.MMDiT(d_model=meta["d"], n_layers=meta["n_layers"], n_heads=meta["n_heads"], mlp_ratio=meta["mlp_ratio"]).eval()
    core.load_state_dict(W["core"], strict=True)
    head = A.MultiModalNoiseHead({"video": meta["d"], "audio": meta["d"]}, {"video": 256, "audio": 32},
                                 hidden_dim=meta["head_hidden"]).eval()
    head.load_state_dict(W["head"], strict=True)
    av = A.LinearAdapter(256, meta["d"] - meta["tdim"])
    aa = A.LinearAdapter(32, meta["d"] - meta["tdim"])
    av.load_state_dict(W["adapt_v"], strict=True)
    aa.load_state_dict(W["adapt_a"], strict=True)
    return core.to(dev), head.to(dev), av.to(dev), aa.to(dev)


def test_block_and_core_golden(dev, small_model):
    g, W, meta = small_model
    core, _, _, _ = _small_modules(dev, W, meta)
    x = G(g["x"], dev)
    assert rel_err(core.blocks[0](x).cpu(), g["y_block0"]) < TOL
    assert rel_err(core(x).cpu(), g["y"]) < TOL
    assert rel_err(core(G(g["x_b"], dev)).cpu(), g["y_b"]) < TOL


def test_head_golden(dev, small_model):
    _, W, meta = small_model
    _, head, _, _ = _small_modules(dev, W, meta)
    g = load_golden("g6_head_small.npz")
    o = head({"video": G(g["hv"], dev), "audio": G(g["ha"], dev)})
    assert rel_err(o["video"].cpu(), g["out_v"]) < TOL
    assert rel_err(o["audio"].cpu(), g["out_a"]) < TOL
    assert torch.equal(head({"video": G(g["hv"], dev)}, return_dict=False), o["video"])


@pytest.mark.parametrize("guide", [0.0, 1.0, 3.5])
@pytest.mark.parametrize("direction", ["a2v", "v2a"])
def test_cfg_step_golden(dev, small_model, guide, direction):
    import multimodal_diffusion_amd as A
    _, W, meta = small_model
    core, head, av, aa = _small_modules(dev, W, meta)
    g = load_golden("g8_cfg_step_small.npz")
    z_v, z_a = G(g["z_v"], dev), G(g["z_a"], dev)
    target = "video" if direction == "a2v" else "audio"
    z_t, z_p = (z_v, z_a) if target == "video" else (z_a, z_v)
    n_prompt = 5 if target == "video" else 8
    eng = A.DenoiseEngine(adapt_v=av, adapt_a=aa, core=core, head=head, tstep_dim=meta["tdim"], target=target,
                          latent_shape=tuple(z_t.shape), prompt_tokens=n_prompt, alpha_bar=T(g["abar"]), guidance=guide)
    eng.set_prompt(z_p)
    zn = eng.step(z_t, G(g["t_now"], dev), G(g["t_prev"], dev))
    e2 = eng.eps_tokens()
    B = z_t.shape[0]
    et = e2[B:] + guide * (e2[:B] - e2[B:])
    assert rel_err(et.cpu(), g[f"{direction}/g{guide}/eps_tok"]) < TOL
    assert rel_err(zn.cpu(), g[f"{direction}/g{guide}/z_next"]) < TOL
    if direction == "a2v" and guide == 3.5:
        assert rel_err(e2[:B].cpu(), g["a2v/eps_cond"]) < TOL
        assert rel_err(e2[B:].cpu(), g["a2v/eps_null"]) < TOL


def test_step_by_module_calls_matches_engine(dev, small_model):
    """The reference's statement-by-statement loop body written with the drop-in modules == the fused engine."""
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import ops, schedule_utils as su
    _, W, meta = small_model
    core, head, av, aa = _small_modules(dev, W, meta)
    g = load_golden("g8_cfg_step_small.npz")
    z_v, z_a, tn, tp = G(g["z_v"], dev), G(g["z_a"], dev), G(g["t_now"], dev), G(g["t_prev"], dev)
    tok_v = A.latents_to_tokens_video(z_v, t_p=2, p=4)
    tok_a = A.latents_to_tokens_audio(z_a, l_chunk=4, s_chunk=4)
    Nv = tok_v.size(1)
    Xv = A.add_sinusoidal_timestep(av(tok_v), tn, meta["tdim"])
    Xa = A.add_sinusoidal_timestep(aa(tok_a), torch.zeros(2, dtype=torch.long, device=dev), meta["tdim"])
    hc = core(torch.cat([Xv, Xa], 1))
    ec = head({"video": hc[:, :Nv], "audio": hc[:, Nv:]})["video"]
    hn = core(torch.cat([Xv, torch.zeros_like(Xa)], 1))
    en = head({"video": hn[:, :Nv], "audio": hn[:, Nv:]})["video"]
    et = en + 3.5 * (ec - en)
    el = ops.tube_unpatch_video(et, C=8, T=4, H=8, W=8, t=2, h=4, w=4)
    zn = su.ddim_step(z_v, tn, tp, el, T(g["abar"]), eta=0.0)
    assert rel_err(zn.cpu(), g["a2v/g3.5/z_next"]) < TOL
    # X holds the sinusoidal embedding at t=982: reproducible to ~1.2e-4 across hosts (see the temb test)
    assert rel_err(torch.cat([Xv, Xa], 1).cpu(), g["a2v/X"]) < 1.2e-4


@pytest.mark.parametrize("graph", [False, True])
def test_chained_sampler_golden(dev, small_model, graph):
    import multimodal_diffusion_amd as A
    _, W, meta = small_model
    core, head, av, aa = _small_modules(dev, W, meta)
    g = load_golden("g9_chain_small.npz")
    eng = A.DenoiseEngine(adapt_v=av, adapt_a=aa, core=core, head=head, tstep_dim=meta["tdim"], target="video",
                          latent_shape=(1, 8, 4, 8, 8), prompt_tokens=5, alpha_bar=T(g["abar"]),
                          guidance=float(g["guidance"]))
    eng.set_prompt(G(g["z_a0"], dev))
    z = eng.run(G(g["z_init"], dev), T(g["sched"]), graph=graph).cpu().double()
    ref = T(g["z_final"]).double()
    assert float((z - ref).norm() / ref.norm()) < 1e-3


# ------------------------------------------------------------------------------------------------- full size
def test_mmdit_full_width(dev, full):
    ws, (core, _, _, _) = full
    x = torch.randn(2, 421, 512, generator=torch.Generator().manual_seed(11))
    ref = R.mmdit_forward(x, ws["core"], 8, 8)
    assert rel_err(core(x.to(dev)).cpu(), ref) < TOL


@pytest.mark.parametrize("size,B", [(32, 4), (64, 2), (256, 2)])
def test_full_step_vs_oracle(dev, full, size, B):
    """configs C1 (32², B=4), C2 shape (64²) and C3 shape (256²) at mvp.yaml model width, one CFG step."""
    ws, (core, head, av, aa) = full
    g = torch.Generator().manual_seed(size)
    z_v = torch.randn(B, 8, 12, size // 8, size // 8, generator=g)
    z_a = torch.randn(B, 8, 150, generator=g)
    abar = R.alpha_bar_table(R.beta_table(1000))
    tn = torch.tensor([982, 500, 16, 999][:B])
    tp = torch.tensor([966, 480, -1, 979][:B])
    ref = R.denoise_step_a2v(z_v, z_a, tn, tp, abar, adapt_v=ws["adapt_v"], adapt_a=ws["adapt_a"], core=ws["core"],
                             head=ws["head"], n_layers=8, n_heads=8, guidance=3.5)
    eng = engine((core, head, av, aa), "video", tuple(z_v.shape), 37, alpha_bar=abar, guidance=3.5)
    eng.set_prompt(z_a.to(dev))
    out = eng.step(z_v.to(dev), tn.to(dev), tp.to(dev)).cpu()
    assert rel_err(out, ref) < TOL


def test_full_step_v2a_vs_oracle(dev, full):
    ws, (core, head, av, aa) = full
    g = torch.Generator().manual_seed(77)
    B = 2
    z_v = torch.randn(B, 8, 12, 16, 16, generator=g)
    z_a = torch.randn(B, 8, 150, generator=g)
    abar = R.alpha_bar_table(R.beta_table(1000))
    tn, tp = torch.tensor([982, 19]), torch.tensor([966, -1])
    ref = R.denoise_step_v2a(z_a, z_v, tn, tp, abar, adapt_v=ws["adapt_v"], adapt_a=ws["adapt_a"], core=ws["core"],
                             head=ws["head"], n_layers=8, n_heads=8, guidance=3.0)
    eng = engine((core, head, av, aa), "audio", tuple(z_a.shape), 96, alpha_bar=abar, guidance=3.0)
    eng.set_prompt(z_v.to(dev))
    assert rel_err(eng.step(z_a.to(dev), tn.to(dev), tp.to(dev)).cpu(), ref) < TOL


def test_trainer_style_add_embedding(dev, full):
    """next-4: adapters of width d with the timestep embedding ADDED (train/trainer.py:45-49) instead of concatenated."""
    import multimodal_diffusion_amd as A
    ws, (core, head, _, _) = full
    g = torch.Generator().manual_seed(21)
    B = 2
    av, aa = A.LinearAdapter(256, 512), A.LinearAdapter(32, 512)
    Wav = {k: v.detach().clone() for k, v in av.state_dict().items()}
    Waa = {k: v.detach().clone() for k, v in aa.state_dict().items()}
    z_v = torch.randn(B, 8, 12, 8, 8, generator=g)
    z_a = torch.randn(B, 8, 150, generator=g)
    abar = R.alpha_bar_table(R.beta_table(1000))
    tn, tp = torch.tensor([982, 500]), torch.tensor([966, 480])
    ref = R.denoise_step_a2v(z_v, z_a, tn, tp, abar, adapt_v=Wav, adapt_a=Waa, core=ws["core"], head=ws["head"], n_layers=8,
                             n_heads=8, guidance=3.0, temb_mode="add")
    eng = A.DenoiseEngine(adapt_v=av.to(dev), adapt_a=aa.to(dev), core=core, head=head, tstep_dim=256, target="video",
                          latent_shape=tuple(z_v.shape), prompt_tokens=37, alpha_bar=abar, guidance=3.0, temb_mode="add")
    eng.set_prompt(z_a.to(dev))
    assert rel_err(eng.step(z_v.to(dev), tn.to(dev), tp.to(dev)).cpu(), ref) < TOL
    with pytest.raises(ValueError):      # concat-mode engine refuses d-wide adapters
        engine((core, head, av, aa), "video", tuple(z_v.shape), 37, alpha_bar=abar, guidance=3.0)


def test_bench_size_properties(dev, full):
    """BASELINE config C3 at full size (256², B=32): properties that need no oracle run.
    - determinism: two runs are bit-identical
    - batch independence: sample b of the B=32 step == the same sample stepped alone (B=1)
    - guidance 0 ignores the prompt; guidance 1 equals the conditional branch"""
    ws, (core, head, av, aa) = full
    g = torch.Generator().manual_seed(1)
    B = 32
    z = torch.randn(B, 8, 12, 32, 32, generator=g).to(dev)
    za = torch.randn(B, 8, 150, generator=torch.Generator().manual_seed(2)).to(dev)
    abar = R.alpha_bar_table(R.beta_table(1000))
    tn = torch.full((B,), 500, device=dev)
    tp = torch.full((B,), 480, device=dev)

    def eng(batch, guide):
        return engine((core, head, av, aa), "video", (batch, 8, 12, 32, 32), 37, alpha_bar=abar, guidance=guide)

    e = eng(B, 3.5)
    e.set_prompt(za)
    o1 = e.step(z, tn, tp)
    o2 = e.step(z, tn, tp)
    assert torch.equal(o1, o2)
    assert torch.isfinite(o1).all()
    e1 = eng(1, 3.5)
    for b in (0, 17, 31):
        e1.set_prompt(za[b:b + 1])
        ob = e1.step(z[b:b + 1].contiguous(), tn[:1], tp[:1])
        assert rel_err(ob.cpu(), o1[b:b + 1].cpu()) < 1e-5
    e0 = eng(B, 0.0)
    e0.set_prompt(za)
    a = e0.step(z, tn, tp)
    e0.set_prompt(torch.flip(za, dims=[0]))
    assert torch.equal(a, e0.step(z, tn, tp))
    eg1 = eng(B, 1.0)
    eg1.set_prompt(za)
    c = eg1.step(z, tn, tp)
    cond = eg1.eps_tokens()[:B]
    from multimodal_diffusion_amd import ops, schedule_utils as su
    lat = ops.tube_unpatch_video(cond, C=8, T=12, H=32, W=32, t=2, h=4, w=4)
    assert rel_err(su.ddim_step(z, tn, tp, lat, abar).cpu(), c.cpu()) < 1e-5


def test_timestep_mlp_golden(dev):
    """TimestepEmbedder(mode='mlp') — sinusoid -> Linear -> SiLU -> Linear, reference state_dict keys."""
    import multimodal_diffusion_amd as A
    g = load_golden("g10_tmlp.npz")
    te = A.TimestepEmbedder(A.TimestepCfg(dim=64, mode="mlp"))
    te.load_state_dict(split_weights(g)["w"], strict=True)
    y = te.to(dev)(G(g["t"], dev)).cpu()
    assert rel_err(y, g["y"]) < 1e-4
    assert rel_err(y, R.timestep_mlp(T(g["t"]), R.cast_weights({"w": split_weights(g)["w"]}, torch.float64)["w"], 64)) < 1e-4
    sin = A.TimestepEmbedder(A.TimestepCfg(dim=64, mode="sin")).to(dev)
    assert torch.equal(sin(G(g["t"], dev)), A.schedule_utils.timestep_embedding(G(g["t"], dev), 64))


def test_errors_are_loud(dev):
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import functional as Fn, _lib as L
    with pytest.raises(L.AvdError):
        Fn.rmsnorm(torch.zeros(2, 8), torch.ones(8))                 # CPU tensor: no fallback
    with pytest.raises(L.AvdError):
        Fn.attention(torch.zeros(1, 4, 3 * 32, device=dev), 1)       # head_dim 32 unsupported
    with pytest.raises(ValueError):
        A.schedule_utils.make_beta_schedule(10, kind="nope")


# ------------------------------------------------------------------------------------------------- VideoVAE.decode (next-1)
def _vae_from(W, dev):
    import multimodal_diffusion_amd as A
    vae = A.VideoVAE.from_config({"latent": {"channels": 8, "t_down": 4, "s_down": 8}}).eval()
    missing, unexpected = vae.load_state_dict(W, strict=False)          # decoder-only weights
    assert not unexpected and all(k.startswith(("enc_net", "to_lat")) for k in missing)
    return vae.to(dev)


def test_vae_decode_golden(dev):
    """Reference VideoVAE.decode (vae_video3d.py:195-214) on a small latent, default and explicit out_size."""
    g = load_golden("g11_vae_decode.npz")
    W = split_weights(g)["w"]
    vae = _vae_from(W, dev)
    x = vae.decode(G(g["z"], dev)).cpu()
    assert x.shape == (2, 3, 8, 32, 32)
    assert rel_err(x, g["x"]) < TOL
    x_odd = vae.decode(G(g["z"][:1], dev), out_size=(6, 24, 40)).cpu()     # ragged tiles: 5760 voxels = 45 tiles
    assert rel_err(x_odd, g["x_odd"]) < TOL
    # chunked batches give the same bits as one batch
    one = vae.decode(G(g["z"], dev), max_workspace_bytes=1).cpu()
    assert torch.equal(one, x)


def test_vae_decode_vs_oracle_bigger(dev):
    """128x128 output (T'=3 -> 12 frames): 196,608 voxels per sample, tanh head, 3 conv blocks, vs the fp64 oracle."""
    import multimodal_diffusion_amd as A
    W = R.synth_vae_decoder(seed=3, n_blocks=3)
    vae = A.VideoVAE(A.VideoVAEConfig(dec_blocks=3, out_activation="tanh")).eval()
    vae.load_state_dict(W, strict=False)
    z = torch.randn(1, 8, 3, 16, 16, generator=torch.Generator().manual_seed(4))
    ref = R.vae_decode(z.double(), {k: v.double() for k, v in W.items()}, n_blocks=3, out_act="tanh")
    x = vae.to(dev).decode(z.to(dev)).cpu()
    assert rel_err(x, ref) < TOL


def test_vae_encode_golden(dev):
    """Reference VideoVAE.encode (vae_video3d.py:164-189): RGB conv on the 4-channel MFMA path, pool + to_lat, crop."""
    import warnings
    import multimodal_diffusion_amd as A
    g = load_golden("g12_vae_encode.npz")
    W = split_weights(g)["w"]
    vae = A.VideoVAE.from_config({"latent": {"channels": 8, "t_down": 4, "s_down": 8}}).eval()
    missing, unexpected = vae.load_state_dict(W, strict=False)
    assert not unexpected and all(k.startswith(("dec_net", "from_lat", "to_img")) for k in missing)
    vae = vae.to(dev)
    z = vae.encode(G(g["x"], dev)).cpu()
    assert z.shape == (2, 8, 2, 2, 3)
    assert rel_err(z, g["z"]) < TOL
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        zc = vae.encode(G(g["x_crop"], dev)).cpu()          # (9,18,17) -> center crop (8,16,16)
    assert rel_err(zc, g["z_crop"]) < TOL
    # encode -> decode shapes compose (the V->A prompt path and the A->V output path)
    assert vae.decode(vae.encode(G(g["x"], dev))).shape == (2, 3, 8, 16, 24)


# ------------------------------------------------------------------------------------------------- AudioCodec (next-2)
def test_audio_codec_golden(dev):
    """Reference AudioCodec.encode / decode (audio_codec.py:184-214) with the shipped hop / frame geometry."""
    from multimodal_diffusion_amd.audio_codec import AudioCodec
    g = load_golden("g13_audio_codec.npz")
    codec = AudioCodec.from_config({"sr": 16000, "latent": {"channels": 8, "frames_per_clip": 150},
                                    "codec": {"hop_samples": 320, "hidden": 64, "smooth_kernel": 7}}).eval()
    codec.load_state_dict(split_weights(g)["w"], strict=True)
    codec = codec.to(dev)
    z = codec.encode(G(g["wav"], dev)).cpu()
    assert z.shape == (2, 8, 150) and rel_err(z, g["z"]) < TOL
    w = codec.decode(G(g["z_in"], dev)).cpu()
    assert w.shape == (2, 1, 3200) and rel_err(w, g["wav_out"]) < TOL
    assert float(w.abs().max()) <= 1.0
    # round 5: the 64 -> 64 layers (k = 9 encoder, k = 7 decoder) run on the fp32 matrix pipe by default — v_mfma_f32_32x32x2_f32 is an fp32
    # FMA chain and the kernel walks (channel, tap) in the vector kernel's order, so the results are BIT-identical (3,200 output positions
    # = 12.5 blocks of 256: the ragged tail; the x 320 upsample is folded into both)
    from multimodal_diffusion_amd import _lib as L
    L.prof_enable(True)
    codec.decode(G(g["z_in"], dev))
    torch.cuda.synchronize()
    L.prof_enable(False)
    assert L.prof_report()["conv1d_mfma_kernel"][0] == 2
    with tuned(codec_mfma=0):
        z0, w0 = codec.encode(G(g["wav"], dev)).cpu(), codec.decode(G(g["z_in"], dev)).cpu()
    L.prof_enable(True)
    try:
        with tuned(codec_mfma=0):
            codec.decode(G(g["z_in"], dev))
            torch.cuda.synchronize()
    finally:
        L.prof_enable(False)
    assert L.prof_report()["conv1d_mfma_kernel"][0] == 0 and L.prof_report()["conv1d_ncl_kernel"][0] == 4
    assert torch.equal(z, z0) and torch.equal(w, w0)


_CODEC_ENV_CHILD = """
import json, sys, torch
from conftest import load_golden, split_weights
from multimodal_diffusion_amd import _lib as L
from multimodal_diffusion_amd.audio_codec import AudioCodec
g = load_golden("g13_audio_codec.npz")
codec = AudioCodec.from_config({"sr": 16000, "latent": {"channels": 8, "frames_per_clip": 150},
                                "codec": {"hop_samples": 320, "hidden": 64, "smooth_kernel": 7}}).eval()
codec.load_state_dict(split_weights(g)["w"], strict=True)
codec = codec.to("cuda:0")
L.prof_enable(True)
codec.decode(torch.from_numpy(g["z_in"]).to("cuda:0"))
torch.cuda.synchronize()
L.prof_enable(False)
print(json.dumps({k: v[0] for k, v in L.prof_report().items() if k.startswith("conv1d")}))
"""


@pytest.mark.gpu_first
def test_tune_key_from_the_environment():
    """The environment path of the tune-key table (csrc/composite.hip): a fresh process started with AVD_CODEC_MFMA=0 decodes the
    golden codec input on the vector kernel only — what avd_tune_set "codec_mfma" 0 selects in test_audio_codec_golden."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    path = [str(ROOT), str(ROOT / "tests")] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]
    env = dict(os.environ, AVD_CODEC_MFMA="0", PYTHONPATH=os.pathsep.join(path))
    r = subprocess.run([sys.executable, "-c", _CODEC_ENV_CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    used = json.loads(r.stdout.strip().splitlines()[-1])
    assert used.get("conv1d_ncl_kernel", 0) > 0 and used.get("conv1d_mfma_kernel", 0) == 0, used


def test_sample_one_direction_end_to_end(dev, full):
    """Reference-signature entry point, both directions, codec + VAE + loop all on HIP, vs the oracle pipeline.
    (The reference's own V->A branch crashes on a permute bug, sample_clip.py:286-289; A->V runs.)"""
    import multimodal_diffusion_amd as A
    ws, mods = full
    vae, codec, cfg = pipeline(dev, seed=3, clip_seconds=0.5, sampler_steps=3, sampling={"ddim_eta": 0.0})
    wav = (0.1 * torch.randn(48000, generator=torch.Generator().manual_seed(5))).numpy()
    kw = dict(components(mods, vae, codec, dev), cfg=cfg)
    torch.manual_seed(77)
    res = A.sample_one_direction(prompt_modality="audio", prompt_video=None, prompt_audio=wav, **kw)
    assert res["video"].shape == (8, 32, 32, 3) and res["video"].dtype == np.uint8 and res["fps"] == 16
    # oracle pipeline on the same draw
    Wc = {k: v.detach().cpu() for k, v in codec.state_dict().items()}
    Wv = {k: v.detach().cpu() for k, v in vae.state_dict().items()}
    torch.manual_seed(77)
    z0 = torch.randn(1, 8, 2, 4, 4, device=dev).cpu()
    z_a0 = R.codec_encode(torch.from_numpy(wav).view(1, 1, -1), Wc)
    abar = R.alpha_bar_table(R.beta_table(1000))
    zf = R.sample_a2v(z0, z_a0, R.sampling_schedule(1000, 3), abar, adapt_v=ws["adapt_v"], adapt_a=ws["adapt_a"], core=ws["core"],
                      head=ws["head"], n_layers=8, n_heads=8, guidance=2.0)
    frames = (R.vae_decode(zf, Wv).clamp(0, 1)[0].permute(1, 2, 3, 0).numpy() * 255.0).astype(np.uint8)
    diff = np.abs(frames.astype(np.int32) - res["video"].astype(np.int32))
    assert diff.max() <= 1 and (diff > 0).mean() < 1e-3        # <= 1 LSB on >= 99.9 % of pixels
    # V -> A with the layout the reference's comment intends, against the oracle PIPELINE on the same draw (VERDICT r4 missing 3):
    # VideoVAE.encode (mean path) -> 3 chained CFG + DDIM steps on the audio latent (sample_clip.py:318-348) -> AudioCodec.decode
    vid = (torch.rand(8, 32, 32, 3, generator=torch.Generator().manual_seed(6)) * 255).to(torch.uint8).numpy()
    z_a_init = torch.randn(1, 8, 150, generator=torch.Generator().manual_seed(78))
    out = A.sample_one_direction(prompt_modality="video", prompt_video=vid, prompt_audio=None, init_noise=z_a_init, **kw)
    assert out["audio"].shape == (48000,) and out["sr"] == 16000 and np.isfinite(out["audio"]).all()
    assert np.abs(out["audio"]).max() <= 1.0
    x_p = (torch.from_numpy(vid).float() / 255.0).permute(3, 0, 1, 2).unsqueeze(0)            # [1,3,T,H,W]
    z_v0 = R.vae_encode(x_p, Wv)
    za_f = R.sample_v2a(z_a_init, z_v0, R.sampling_schedule(1000, 3), abar, adapt_v=ws["adapt_v"], adapt_a=ws["adapt_a"], core=ws["core"],
                        head=ws["head"], n_layers=8, n_heads=8, guidance=2.0)
    wav_ref = R.codec_decode(za_f, Wc)[0, 0].double()
    l2 = float((torch.from_numpy(out["audio"]).double() - wav_ref).norm() / wav_ref.norm())
    assert l2 < 1e-3, l2                      # chained tolerance
    with pytest.raises(ValueError):
        A.sample_one_direction(prompt_modality="video", prompt_video=vid, prompt_audio=None, init_noise=torch.zeros(1, 8, 149), **kw)
    with pytest.raises(ValueError):
        A.sample_one_direction(prompt_modality="smell", prompt_video=None, prompt_audio=wav, **kw)


@pytest.mark.parametrize("mode", ["f32", "bf16x3", "auto"])
def test_sample_one_direction_shipped_config_golden(dev, mode):
    """Fixture g19 (VERDICT r4 missing 4): the reference's OWN sample_one_direction(prompt_modality="audio") on its unmodified shipped
    configuration (configs/mvp.yaml + a2v.yaml: d = 512, L = 8, 128 x 128 x 48 frames, 60 DDIM steps, g = 3.5) — here through the mirror
    entry point with the same config, the same seeded-recipe weights and the same initial latent: codec encode, 60 chained steps, VideoVAE
    decode, uint8 frames, all on HIP.  "bf16x3" forces the split-operand kernels at this 266-row batch (they engage at 2,048 by default)."""
    import multimodal_diffusion_amd as A
    from test_oracle_golden import frames_close, g19_setup
    g, meta, ws, Wv, Wc, wav = g19_setup()
    cfg = dict(meta["cfg"], runtime={"matmul": mode})
    vae, codec, av, aa, core, head, tdim = A.build_components(cfg, dev)
    core.load_state_dict(ws["core"], strict=True)
    head.load_state_dict(ws["head"], strict=True)
    av.load_state_dict(ws["adapt_v"], strict=True)
    aa.load_state_dict(ws["adapt_a"], strict=True)
    vae.load_state_dict(Wv, strict=True)
    codec.load_state_dict(Wc, strict=True)
    rec = {}
    dec0 = vae.decode
    vae.decode = lambda z, *a, **k: (rec.__setitem__("z", z.clone()), dec0(z, *a, **k))[1]
    with tuned("s3_min_rows"):
        if mode == "bf16x3":
            tune("s3_min_rows", 0)
        res = A.sample_one_direction(cfg=cfg, vid_vae=vae, aud_codec=codec, adapt_v=av, adapt_a=aa, core=core, head=head, tstep_dim=tdim,
                                     prompt_modality="audio", prompt_video=None, prompt_audio=wav, device=dev, init_noise=T(g["z_init"]))
    ref = T(g["z_final"]).double()
    l2 = float((rec["z"].cpu().double() - ref).norm() / ref.norm())
    assert l2 < 1e-3, (mode, l2)              # chained tolerance
    assert res["video"].shape == (48, 128, 128, 3) and res["video"].dtype == np.uint8 and res["fps"] == 16
    mx, frac = frames_close(res["video"][::meta["frame_stride"]], g["frames"])
    assert mx <= 1 and frac < 1e-3, (mode, mx, frac)      # <= 1 LSB on >= 99.9 % of the pixels


@pytest.mark.parametrize("mode", ["f32", "bf16x3", "f16x2", "auto"])
def test_chain_full_width_vs_oracle(dev, full, mode):
    """A 10-step DDIM + CFG trajectory at the C3 shape (256 x 256: 384 + 37 tokens, d = 512, L = 8) at batch 4 against the CPU ORACLE's
    chain (R.sample_a2v) — not against another mode of this library (VERDICT r4 missing 4 / next-round 5c).  3,368 rows: "auto" and
    "bf16x3" take the six-term split kernels, "f16x2" needs its row threshold lowered."""
    from multimodal_diffusion_amd import schedule_utils as su
    ws, _ = full
    B = 4
    g = torch.Generator().manual_seed(1010)
    z = torch.randn(B, 8, 12, 32, 32, generator=g)
    za = torch.randn(B, 8, 150, generator=g)
    abar = R.alpha_bar_table(R.beta_table(1000))
    sched = su.make_sampling_schedule(1000, 10)
    ref = R.sample_a2v(z, za, R.sampling_schedule(1000, 10), abar, adapt_v=ws["adapt_v"], adapt_a=ws["adapt_a"], core=ws["core"],
                       head=ws["head"], n_layers=8, n_heads=8, guidance=3.5).double()
    core, head, av, aa = modules(dev, ws, 8)
    with tuned("s3_min_rows"):
        if mode == "f16x2":
            tune("s3_min_rows", 0)
        eng = engine((core, head, av, aa), "video", tuple(z.shape), 37, alpha_bar=abar, guidance=3.5, matmul=mode)
        eng.set_prompt(za.to(dev))
        out = eng.run(z.to(dev), sched)
    l2 = float((out.cpu().double() - ref).norm() / ref.norm())
    assert torch.isfinite(out).all() and l2 < 1e-3, (mode, l2)       # chained tolerance; final |z| ~ 1e4


# ------------------------------------------------------------------------------------------------- stream_infer (next-3)
def test_crossfade_golden_bit_exact(dev):
    from multimodal_diffusion_amd import stream_infer as S
    g = load_golden("g14_stream_stitch.npz")
    assert np.array_equal(S.crossfade_audio(g["a_chunks"], sr=1000, hop=400, win=1000, fade_s=0.25, device=dev), g["a_fade"])
    assert np.array_equal(S.crossfade_audio(g["a_chunks"], sr=1000, hop=400, win=1000, fade_s=0.0, device=dev), g["a_rect"])
    assert np.array_equal(S.crossfade_video(g["v_chunks"], hop=4, win=12, fade_f=3, device=dev), g["v_fade"])
    assert np.array_equal(S.crossfade_video(g["v_chunks"], hop=4, win=12, fade_f=0, device=dev), g["v_rect"])


def test_stream_generate_equals_per_window_sampling(dev, full):
    """All windows batched through one engine == the reference's per-window loop + cross-fade (same initial latents)."""
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import stream_infer as S
    ws, (core, head, av, aa) = full
    vae, codec, cfg = pipeline(dev, seed=8, clip_seconds=0.5, sampler_steps=2, streaming=STREAM_HALF_SECOND,
                               sampling={"ddim_eta": 0.0})
    wav = (0.1 * torch.randn(18000, generator=torch.Generator().manual_seed(9))).numpy()
    kw = dict(components((core, head, av, aa), vae, codec, dev), cfg=cfg)
    chunks, win, hop = S.split_audio_into_windows(wav, sr=16000, win_s=0.5, hop_s=0.25)
    noise = torch.randn(chunks.shape[0], 8, 2, 4, 4, generator=torch.Generator().manual_seed(10))
    out = S.stream_generate(prompt_modality="audio", prompt_video=None, prompt_audio=wav, init_noise=noise, **kw)
    # per-window reference flow with the product's single-window entry point pieces
    per = []
    abar = A.schedule_utils.alphas_cumprod_from_betas(A.schedule_utils.make_beta_schedule(1000))[1]
    sched = A.schedule_utils.make_sampling_schedule(1000, 2)
    for i in range(chunks.shape[0]):
        z_p = codec.encode(torch.from_numpy(chunks[i]).to(dev).view(1, 1, -1))
        eng = engine((core, head, av, aa), "video", (1, 8, 2, 4, 4), 37, alpha_bar=abar, guidance=2.0)
        eng.set_prompt(z_p)
        x = vae.decode(eng.run(noise[i:i + 1].to(dev), sched)).clamp(0, 1)
        per.append((x[0].permute(1, 2, 3, 0).cpu().numpy() * 255.0).astype(np.uint8))
    ref = R.crossfade(np.stack(per).astype(np.float32) / 255.0, S.video_fade_window(8, 2), 4)
    ref = (np.clip(ref, 0, 1) * 255.0).astype(np.uint8)
    assert out["video"].shape == ref.shape and out["fps"] == 16
    d = np.abs(out["video"].astype(np.int32) - ref.astype(np.int32))
    assert d.max() <= 1 and (d > 0).mean() < 1e-3


# ------------------------------------------------------------------------------------------------- bf16x3 matmul path
@pytest.mark.parametrize("rows,K", [(5, 16), (300, 512), (1000, 2048)])
def test_split3_is_exact(dev, rows, K):
    """x == h + m + l exactly (each plane 8 significant bits), including huge and tiny magnitudes."""
    from multimodal_diffusion_amd import functional as Fn
    g = torch.Generator().manual_seed(rows + K)
    x = torch.randn(rows, K, generator=g) * torch.exp(torch.randn(rows, 1, generator=g) * 6.0)
    img = Fn.split3(x.to(dev)).cpu().numpy()
    pl = _split3_decode(img, rows, K).astype(np.float64)
    assert np.array_equal(pl.sum(0), x.numpy().astype(np.float64))
    assert np.abs(pl[1]).max() <= np.abs(pl[0]).max() * 2.0 ** -8 and np.abs(pl[2]).max() <= np.abs(pl[0]).max() * 2.0 ** -16


@pytest.mark.parametrize("M,N,K", [(700, 512, 256), (333, 768, 2048), (5000, 1536, 512), (130, 256, 16)])
@pytest.mark.parametrize("mode", ["plain", "res", "gelu_split"])
def test_gemm_bf16x3_fp32_accuracy(dev, M, N, K, mode):
    """The split-operand GEMM must be as accurate as the fp32 MFMA GEMM: both are compared with an fp64 result."""
    from multimodal_diffusion_amd import functional as Fn, _lib as L
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g) * 3.0
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    b = torch.randn(N, generator=g)
    r = torch.randn(M, N, generator=g)
    ref = R.linear(x.double(), w.double(), b.double())
    x3, w3 = Fn.split3(x.to(dev)), Fn.split3(w.to(dev))
    if mode == "gelu_split":
        ref = R.gelu_erf(ref)
        img = Fn.linear_bf16x3(x3, M, w3, N, K, bias=b.to(dev), act=L.ACT_GELU, out_split3=True).cpu().numpy()
        y = torch.from_numpy(_split3_decode(img, M, N).astype(np.float64).sum(0))
        y32 = Fn.linear(x.to(dev), w.to(dev), b.to(dev), act=L.ACT_GELU).cpu()
    else:
        if mode == "res":
            ref = ref + r.double()
        y = Fn.linear_bf16x3(x3, M, w3, N, K, bias=b.to(dev), residual=r.to(dev) if mode == "res" else None).cpu()
        y32 = Fn.linear(x.to(dev), w.to(dev), b.to(dev), residual=r.to(dev) if mode == "res" else None).cpu()
    e3 = (y.double() - ref).abs().max().item()
    e32 = (y32.double() - ref).abs().max().item()
    assert e3 <= 2e-6 * ref.abs().max().item()
    assert e3 <= 1.5 * e32 + 1e-7, (e3, e32)


def test_rmsnorm_split3(dev):
    from multimodal_diffusion_amd import functional as Fn
    g = torch.Generator().manual_seed(3)
    x = torch.randn(777, 512, generator=g)
    x[5] *= 1e-7
    s = torch.rand(512, generator=g) + 0.5
    img = Fn.rmsnorm_split3(x.to(dev), s.to(dev), 1e-6).cpu().numpy()
    y = _split3_decode(img, 777, 512).astype(np.float64).sum(0)
    assert rel_err(torch.from_numpy(y), R.rmsnorm(x.double(), s.double(), 1e-6)) < 1e-6
    assert rel_err(torch.from_numpy(y), Fn.rmsnorm(x.to(dev), s.to(dev), 1e-6).cpu()) < 1e-6


def test_core_bf16x3_vs_oracle_and_f32(dev, full):
    """MMDiT.forward at a batch large enough for the bf16x3 path (rows >= 6144): same tolerance as the fp32 path, and
    no further from the fp64 oracle than the fp32 MFMA path is."""
    ws, _ = full
    core3, _, _, _ = modules(dev, ws, 8)
    core32, _, _, _ = modules(dev, ws, 8)
    core3.matmul, core32.matmul = "bf16x3", "f32"
    x = torch.randn(40, 421, 512, generator=torch.Generator().manual_seed(12))
    y3 = core3(x.to(dev)).cpu()
    y32 = core32(x.to(dev)).cpu()
    assert not torch.equal(y3, y32), "bf16x3 path did not run"
    sub = slice(0, 3)
    ref = R.mmdit_forward(x[sub].double(), {k: v.double() for k, v in ws["core"].items()}, 8, 8)
    e3, e32 = rel_err(y3[sub], ref), rel_err(y32[sub], ref)
    assert e3 < TOL and e32 < TOL
    assert e3 < 2.0 * e32 + 1e-7, (e3, e32)
    assert rel_err(y3, y32) < 2e-5


def test_full_step_bf16x3_vs_oracle(dev, full):
    """BASELINE C3 shape, B=20 (2B*N = 16,840 rows, the bf16x3 path), one CFG step against the CPU oracle."""
    ws, _ = full
    core, head, av, aa = modules(dev, ws, 8)
    B = 20
    g = torch.Generator().manual_seed(256)
    z_v = torch.randn(B, 8, 12, 32, 32, generator=g)
    z_a = torch.randn(B, 8, 150, generator=g)
    abar = R.alpha_bar_table(R.beta_table(1000))
    tn = torch.tensor([982, 500, 16, 999] * 5)
    tp = torch.tensor([966, 480, -1, 979] * 5)
    nb = 4                                                          # oracle on the first samples only (samples are independent)
    ref = R.denoise_step_a2v(z_v[:nb], z_a[:nb], tn[:nb], tp[:nb], abar, adapt_v=ws["adapt_v"], adapt_a=ws["adapt_a"],
                             core=ws["core"], head=ws["head"], n_layers=8, n_heads=8, guidance=3.5)
    eng = engine((core, head, av, aa), "video", tuple(z_v.shape), 37, alpha_bar=abar, guidance=3.5, matmul="bf16x3")
    assert eng.matmul == "bf16x3"
    eng.set_prompt(z_a.to(dev))
    out = eng.step(z_v.to(dev), tn.to(dev), tp.to(dev))
    assert torch.equal(out, eng.step(z_v.to(dev), tn.to(dev), tp.to(dev)))        # deterministic
    assert rel_err(out[:nb].cpu(), ref) < TOL


def test_attention_split3_output(dev):
    """The attention kernel's split3 epilogue holds exactly the fp32 values of the plain kernel."""
    import ctypes as C
    from multimodal_diffusion_amd import functional as Fn, _lib as L
    B, N, H = 3, 133, 8
    qkv = torch.randn(B, N, 3 * H * 64, generator=torch.Generator().manual_seed(5)).to(dev)
    ref = Fn.attention(qkv, H).cpu().double().numpy().reshape(B * N, H * 64)
    img = torch.zeros(L.lib().avd_split3_bytes(B * N, H * 64), dtype=torch.uint8, device=dev)
    L.check(L.lib().avd_attn_fwd_split3_f32(qkv.data_ptr(), img.data_ptr(), B, N, H, 64, 0.125, N, L.stream_ptr(dev)))
    got = _split3_decode(img.cpu().numpy(), B * N, H * 64).astype(np.float64).sum(0)
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("B,N,H", [(2, 133, 4), (1, 421, 4), (3, 64, 8), (2, 37, 4)])
def test_attention_bf16x3(dev, B, N, H):
    """in_proj epilogue -> qkv3 image -> bf16x3 attention, against softmax(q k^T / 8) v in fp64 and against the fp32-MFMA kernel."""
    from multimodal_diffusion_amd import functional as Fn, _lib as L
    d = H * 64
    g = torch.Generator().manual_seed(B * 1000 + N + H)
    qkv = torch.randn(B * N, 3 * d, generator=g) * 1.5
    bias = torch.randn(3 * d, generator=g) * 0.1
    lib = L.lib()
    img = torch.empty(lib.avd_qkv3_bytes(B, N, H), dtype=torch.uint8, device=dev)
    x3, w3 = Fn.split3(qkv.to(dev)), Fn.split3(torch.eye(3 * d).to(dev))      # identity in_proj: the image holds qkv + bias exactly
    bd = bias.to(dev)
    L.check(lib.avd_gemm_bf16x3_qkv3_f32(x3.data_ptr(), w3.data_ptr(), bd.data_ptr(), img.data_ptr(), B * N, N, H, 3 * d,
                                         0.125 * 1.4426950408889634, 6, L.stream_ptr(dev)))
    out = torch.empty(B, N, d, device=dev)
    L.check(lib.avd_attn_fwd_qkv3_f32(img.data_ptr(), out.data_ptr(), None, B, N, H, N, 6, L.stream_ptr(dev)))
    full = (qkv + bias).double().view(B, N, 3, H, 64)
    q, k, v = (full[:, :, i].transpose(1, 2) for i in range(3))                  # [B,H,N,64]
    ref = (torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1) @ v).transpose(1, 2).reshape(B, N, d)
    e3 = rel_err(out.cpu(), ref)
    e32 = rel_err(Fn.attention((qkv + bias).view(B, N, 3 * d).to(dev), H).cpu(), ref)
    assert e3 < 2e-6 and e3 < 2.0 * e32 + 2e-7, (e3, e32)
    # split3-image output == fp32 output; n_query leaves later rows untouched
    o3 = torch.zeros(lib.avd_split3_bytes(B * N, d), dtype=torch.uint8, device=dev)
    nq = max(1, N - 5)
    L.check(lib.avd_attn_fwd_qkv3_f32(img.data_ptr(), None, o3.data_ptr(), B, N, H, nq, 6, L.stream_ptr(dev)))
    got = _split3_decode(o3.cpu().numpy(), B * N, d).astype(np.float64).sum(0).reshape(B, N, d)
    assert np.array_equal(got[:, :nq], out.cpu().double().numpy()[:, :nq])
    assert not got[:, nq:].any()


def test_chain_bf16x3_tracks_f32(dev, full):
    """A 10-step DDIM + CFG trajectory at the C3 shape (B=20): the bf16x3 matmul mode stays within the chained tolerance of
    the fp32-MFMA mode (rel L2 <= 1e-3) — eager and as a replayed HIP graph."""
    from multimodal_diffusion_amd import schedule_utils as su
    ws, _ = full
    B = 20
    g = torch.Generator().manual_seed(99)
    z = torch.randn(B, 8, 12, 32, 32, generator=g).to(dev)
    za = torch.randn(B, 8, 150, generator=g).to(dev)
    abar = R.alpha_bar_table(R.beta_table(1000))
    sched = su.make_sampling_schedule(1000, 10)
    outs = {}
    for mode in ("f32", "bf16x3"):
        core, head, av, aa = modules(dev, ws, 8)
        eng = engine((core, head, av, aa), "video", tuple(z.shape), 37, alpha_bar=abar, guidance=3.5, matmul=mode)
        eng.set_prompt(za)
        outs[mode] = eng.run(z, sched)
        if mode == "bf16x3":
            outs["bf16x3_graph"] = eng.run(z, sched, graph=True)
    ref = outs["f32"].double()
    for k in ("bf16x3", "bf16x3_graph"):
        l2 = float((outs[k].double() - ref).norm() / ref.norm())
        assert l2 < 1e-3, (k, l2)
    assert torch.equal(outs["bf16x3"], outs["bf16x3_graph"])


def test_full_step_bf16x3_512(dev, full):
    """BASELINE C5 geometry (512x512: 1536+37 tokens, ragged 1573 -> 1600 padded keys), B=6 -> 18,876 rows on the bf16x3 path."""
    ws, _ = full
    core, head, av, aa = modules(dev, ws, 8)
    B = 6
    g = torch.Generator().manual_seed(512)
    z_v = torch.randn(B, 8, 12, 64, 64, generator=g)
    z_a = torch.randn(B, 8, 150, generator=g)
    abar = R.alpha_bar_table(R.beta_table(1000))
    tn = torch.tensor([982, 500, 16, 999, 700, 300])
    tp = torch.tensor([966, 480, -1, 979, 680, 280])
    ref = R.denoise_step_a2v(z_v[:1], z_a[:1], tn[:1], tp[:1], abar, adapt_v=ws["adapt_v"], adapt_a=ws["adapt_a"],
                             core=ws["core"], head=ws["head"], n_layers=8, n_heads=8, guidance=3.5)
    eng = engine((core, head, av, aa), "video", tuple(z_v.shape), 37, alpha_bar=abar, guidance=3.5, matmul="bf16x3")
    eng.set_prompt(z_a.to(dev))
    out = eng.step(z_v.to(dev), tn.to(dev), tp.to(dev))
    assert rel_err(out[:1].cpu(), ref) < TOL


@pytest.mark.parametrize("M,N,K", [(1, 256, 16), (255, 256, 64), (256, 512, 4096), (257, 256, 512), (513, 768, 48)])
def test_gemm_bf16x3_edge_shapes(dev, M, N, K):
    """Row counts around the 128/256-row tile edges, the smallest and a large K."""
    from multimodal_diffusion_amd import functional as Fn
    g = torch.Generator().manual_seed(M * 3 + N + K)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    b = torch.randn(N, generator=g)
    r = torch.randn(M, N, generator=g)
    ref = R.linear(x.double(), w.double(), b.double()) + r.double()
    y = Fn.linear_bf16x3(Fn.split3(x.to(dev)), M, Fn.split3(w.to(dev)), N, K, bias=b.to(dev), residual=r.to(dev)).cpu()
    assert rel_err(y, ref) < 2e-6


@pytest.mark.parametrize("B,N,H,nq", [(1, 5, 4, 5), (2, 64, 4, 64), (1, 200, 4, 1), (1, 129, 8, 128), (1, 1573, 4, 1536)])
def test_attention_bf16x3_edge_shapes(dev, B, N, H, nq):
    """Sequences shorter than a key tile, exactly one tile, ragged long (the 512x512 geometry) and tiny / ragged query counts."""
    from multimodal_diffusion_amd import functional as Fn, _lib as L
    d = H * 64
    g = torch.Generator().manual_seed(N + H)
    qkv = torch.randn(B * N, 3 * d, generator=g)
    lib = L.lib()
    img = torch.empty(lib.avd_qkv3_bytes(B, N, H), dtype=torch.uint8, device=dev)
    x3, w3 = Fn.split3(qkv.to(dev)), Fn.split3(torch.eye(3 * d).to(dev))
    zb = torch.zeros(3 * d, device=dev)
    L.check(lib.avd_gemm_bf16x3_qkv3_f32(x3.data_ptr(), w3.data_ptr(), zb.data_ptr(), img.data_ptr(), B * N, N, H, 3 * d,
                                         0.125 * 1.4426950408889634, 6, L.stream_ptr(dev)))
    out = torch.full((B, N, d), 7.0, device=dev)
    L.check(lib.avd_attn_fwd_qkv3_f32(img.data_ptr(), out.data_ptr(), None, B, N, H, nq, 6, L.stream_ptr(dev)))
    full = qkv.double().view(B, N, 3, H, 64)
    q, k, v = (full[:, :, i].transpose(1, 2) for i in range(3))
    ref = (torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1) @ v).transpose(1, 2).reshape(B, N, d)
    assert rel_err(out.cpu()[:, :nq], ref[:, :nq]) < 2e-6
    assert torch.all(out[:, nq:] == 7.0)


@pytest.mark.parametrize("B,N,H,nq,terms", [(2, 133, 4, 133, 6), (1, 421, 8, 421, 6), (3, 64, 8, 64, 6), (2, 37, 4, 37, 6), (1, 5, 4, 5, 6),
                                             (1, 200, 4, 1, 6), (1, 129, 8, 128, 6), (1, 1573, 4, 1536, 6), (2, 421, 4, 384, 9), (2, 257, 4, 257, 1)])
def test_attention_m16_shape(dev, B, N, H, nq, terms):
    """Round 5: the split-operand attention on v_mfma_f32_16x16x32 (avd_tune_set "attn_m16"; attn_bf16x3_p16_kernel — query columns spread
    over the four 16-lane groups, V read in the key order two S^T tiles give): against softmax(q k^T / 8) v in fp64 at the 32x32x16 kernel's
    tolerance, next to that kernel's own error, rows past n_query untouched, and the operand-image output equal to the fp32 output."""
    from multimodal_diffusion_amd import functional as Fn, _lib as L
    d = H * 64
    g = torch.Generator().manual_seed(N * 7 + H + terms)
    qkv = torch.randn(B * N, 3 * d, generator=g) * 1.5
    lib = L.lib()
    img = torch.empty(lib.avd_qkv3_bytes(B, N, H), dtype=torch.uint8, device=dev)
    x3, w3 = Fn.split3(qkv.to(dev)), Fn.split3(torch.eye(3 * d).to(dev))
    zb = torch.zeros(3 * d, device=dev)
    L.check(lib.avd_gemm_bf16x3_qkv3_f32(x3.data_ptr(), w3.data_ptr(), zb.data_ptr(), img.data_ptr(), B * N, N, H, 3 * d,
                                         0.125 * 1.4426950408889634, 6, L.stream_ptr(dev)))
    full = qkv.double().view(B, N, 3, H, 64)
    q, k, v = (full[:, :, i].transpose(1, 2) for i in range(3))
    ref = (torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1) @ v).transpose(1, 2).reshape(B, N, d)
    outs = {}
    with tuned("attn_m16"):
        for m16 in (0, 2):
            tune("attn_m16", m16)
            out = torch.full((B, N, d), 7.0, device=dev)
            L.check(lib.avd_attn_fwd_qkv3_f32(img.data_ptr(), out.data_ptr(), None, B, N, H, nq, terms, L.stream_ptr(dev)))
            outs[m16] = out.cpu()
        o3 = torch.zeros(lib.avd_split3_bytes(B * N, d), dtype=torch.uint8, device=dev)
        L.check(lib.avd_attn_fwd_qkv3_f32(img.data_ptr(), None, o3.data_ptr(), B, N, H, nq, terms, L.stream_ptr(dev)))
    tol = 2e-6 if terms != 1 else 2e-2          # (one plane: plain bf16 operands, reduced precision)
    e16, e32 = rel_err(outs[2][:, :nq], ref[:, :nq]), rel_err(outs[0][:, :nq], ref[:, :nq])
    assert e16 < tol and e16 < 2.0 * e32 + 2e-7, (e16, e32)
    assert torch.all(outs[2][:, nq:] == 7.0)
    got = _split3_decode(o3.cpu().numpy(), B * N, d).astype(np.float64).sum(0).reshape(B, N, d)
    assert np.array_equal(got[:, :nq], outs[2].double().numpy()[:, :nq]) and not got[:, nq:].any()


def test_vae_decode_bf16x3(dev):
    """Decoder convolutions on the bf16 matrix pipe with split operands: golden fixture, ragged tiles, and the fp64 oracle at
    128x128 — same tolerance as the fp32-MFMA decoder, and no further from fp64 than that decoder is."""
    import multimodal_diffusion_amd as A
    g = load_golden("g11_vae_decode.npz")
    vae = _vae_from(split_weights(g)["w"], dev)
    vae.matmul = "bf16x3"
    x = vae.decode(G(g["z"], dev)).cpu()
    assert rel_err(x, g["x"]) < TOL
    assert rel_err(vae.decode(G(g["z"][:1], dev), out_size=(6, 24, 40)).cpu(), g["x_odd"]) < TOL
    assert torch.equal(vae.decode(G(g["z"], dev), max_workspace_bytes=1).cpu(), x)
    W = R.synth_vae_decoder(seed=3, n_blocks=3)
    z = torch.randn(1, 8, 3, 16, 16, generator=torch.Generator().manual_seed(4))
    ref = R.vae_decode(z.double(), {k: v.double() for k, v in W.items()}, n_blocks=3, out_act="tanh")
    errs = {}
    for mode in ("f32", "bf16x3"):
        v = A.VideoVAE(A.VideoVAEConfig(dec_blocks=3, out_activation="tanh")).eval()
        v.load_state_dict(W, strict=False)
        v.matmul = mode
        errs[mode] = rel_err(v.to(dev).decode(z.to(dev)).cpu(), ref)
    assert errs["bf16x3"] < TOL and errs["bf16x3"] < 2.0 * errs["f32"] + 1e-7, errs


@pytest.mark.parametrize("mode", ["bf16x3", "f16x2"])
def test_vae_decode_latent_composed_first_conv(dev, mode):
    """Round 5: in the split-operand modes the decoder's first convolution runs on upsample(z) with composite weights (from_lat folded
    into dec_net.0.0: 8 input channels instead of 64, one 16-channel slab of 27 taps; from_lat's bias through a border-class table —
    VideoVAE._lat_composite, conv3d_k3_bf16x3_kernel<.., 1>).  Same operator as from_lat -> upsample -> 64-channel conv up to fp32
    rounding: against that route (lat_composed = False), against the golden fixture (also the ragged output size, whose border voxels
    take the border rows of the bias table) and against the fp64 oracle on a decoder with a large from_lat bias."""
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import _lib as L
    g = load_golden("g11_vae_decode.npz")
    outs = {}
    for lat in (False, True, "one tap per step"):           # True: two taps per k-step (lat_ch = 8: ABI 7 conv0_lat_packed), the default
        vae = _vae_from(split_weights(g)["w"], dev)
        vae.matmul, vae.lat_composed, vae.lat_packed = mode, bool(lat), lat is True
        L.prof_enable(True)
        x = vae.decode(G(g["z"], dev)).cpu()
        torch.cuda.synchronize()
        L.prof_enable(False)
        used = {k for k, v in L.prof_report().items() if v[0] > 0}
        assert any(re.match(r"conv3d_k3_bf16x3_kernel<\d, %s, \d>" % ("0" if lat is True else "1"), k) for k in used) == bool(lat), used
        assert ("upsample_lat8_kernel" in used) == bool(lat) and ("fromlat_kernel" in used) == (not lat), used      # lat_ch = 8: channel-last latent
        outs[lat] = (x, vae.decode(G(g["z"][:1], dev), out_size=(6, 24, 40)).cpu())
    for lat in (True, "one tap per step"):
        assert rel_err(outs[lat][0], g["x"]) < TOL and rel_err(outs[lat][1], g["x_odd"]) < TOL
        assert rel_err(outs[lat][0], outs[False][0]) < 2e-5 and rel_err(outs[lat][1], outs[False][1]) < 2e-5
    # a decoder whose from_lat bias dominates: the border table carries real weight (tiny volume: every voxel class occurs)
    W = R.synth_vae_decoder(seed=5, n_blocks=2)
    W["from_lat.bias"] = W["from_lat.bias"] * 0 + torch.linspace(-3.0, 3.0, 64)
    z = torch.randn(2, 8, 1, 2, 3, generator=torch.Generator().manual_seed(6))
    ref = R.vae_decode(z.double(), {k: v.double() for k, v in W.items()}, n_blocks=2)
    errs = {}
    for lat in (False, True):
        v = A.VideoVAE(A.VideoVAEConfig(dec_blocks=2)).eval()
        v.load_state_dict(W, strict=False)
        v.matmul, v.lat_composed = mode, lat
        errs[lat] = rel_err(v.to(dev).decode(z.to(dev)).cpu(), ref)
    assert errs[True] < TOL and errs[True] < 2.0 * errs[False] + 1e-6, errs


@pytest.mark.parametrize("mode", ["bf16x3", "f16x2"])
def test_vae_decode_folded_route(dev, mode):
    """Round 5 (f16x2: the to_img part only — an fp16 image of conv 0's output would need a bound on values that do not exist yet).
    bf16x3, two conv blocks, latent-composed first conv: conv 0 writes GELU(y) straight into conv 1's operand image, the
    GroupNorm between them (vae_video3d.py:81-83) is folded into conv 1's per-sample weights and a border-class bias table, and to_img
    (:210-214) is finished from per-group partial sums of conv 1's epilogue — no fp32 activation buffer between the kernels
    (avd_tune_set "vae_fold").  Same operator up to fp32 rounding: against the other route, the golden fixture (two samples = two sets
    of statistics; the ragged size, whose border voxels take the border rows of the tables), and the fp64 oracle on a decoder built
    to stress the fold — a conv 0 bias that puts the activations' mean far above their spread (GN's subtraction then happens through
    the table) with GroupNorm weights and shifts of order one."""
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import _lib as L
    g = load_golden("g11_vae_decode.npz")
    outs = {}
    with tuned("vae_fold"):
        for fold in (0, 1):
            tune("vae_fold", fold)
            vae = _vae_from(split_weights(g)["w"], dev)
            vae.matmul = mode
            L.prof_enable(True)
            x = vae.decode(G(g["z"], dev)).cpu()
            torch.cuda.synchronize()
            L.prof_enable(False)
            used = {k for k, v in L.prof_report().items() if v[0] > 0}
            want = {"conv3d_k3_bf16x3_kernel<6, 0, 1>", "conv3d_k3_bf16x3_kernel<6, 4, 2>", "toimg_from_p_kernel"} if mode == "bf16x3" else \
                   {"conv3d_k3_bf16x3_kernel<3, 4, 2>", "toimg_from_p_kernel"}
            assert (want <= used) == bool(fold), used
            assert ("gn_apply_toimg_kernel" in used) == (not fold) and ("gn_apply_pad3_kernel" in used) == (not fold or mode == "f16x2"), used
            outs[fold] = (x, vae.decode(G(g["z"][:1], dev), out_size=(6, 24, 40)).cpu())
        assert rel_err(outs[1][0], g["x"]) < TOL and rel_err(outs[1][1], g["x_odd"]) < TOL
        assert rel_err(outs[1][0], outs[0][0]) < 2e-5 and rel_err(outs[1][1], outs[0][1]) < 2e-5
        W = R.synth_vae_decoder(seed=7, n_blocks=2)
        gen = torch.Generator().manual_seed(8)
        W["dec_net.0.0.bias"] = 1.5 + 0.5 * torch.rand(64, generator=gen)
        for i in (0, 1):
            W[f"dec_net.{i}.2.weight"] = torch.randn(64, generator=gen)
            W[f"dec_net.{i}.2.bias"] = torch.randn(64, generator=gen)
        z = torch.randn(3, 8, 1, 2, 3, generator=gen)
        ref = R.vae_decode(z.double(), {k: v.double() for k, v in W.items()}, n_blocks=2)
        errs = {}
        for fold in (0, 1):
            tune("vae_fold", fold)
            v = A.VideoVAE(A.VideoVAEConfig(dec_blocks=2)).eval()
            v.load_state_dict(W, strict=False)
            v.matmul = mode
            errs[fold] = rel_err(v.to(dev).decode(z.to(dev)).cpu(), ref)
        assert errs[1] < TOL and errs[1] < 3.0 * errs[0] + 1e-6, errs


def test_vae_encode_bf16x3(dev):
    """Encoder with its 64 -> 64 convolution(s) on the bf16x3 path: golden fixture at the fp32 encoder's tolerance."""
    import warnings
    import multimodal_diffusion_amd as A
    g = load_golden("g12_vae_encode.npz")
    vae = A.VideoVAE.from_config({"latent": {"channels": 8, "t_down": 4, "s_down": 8}}).eval()
    vae.load_state_dict(split_weights(g)["w"], strict=False)
    vae = vae.to(dev)
    vae.matmul = "f32"
    z32 = vae.encode(G(g["x"], dev)).cpu()
    vae.matmul = "bf16x3"
    z3 = vae.encode(G(g["x"], dev)).cpu()
    assert rel_err(z3, g["z"]) < TOL and rel_err(z3, z32) < 2e-5
    assert not torch.equal(z3, z32) or len(vae.enc_net) == 1, "bf16x3 encoder path did not run"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert rel_err(vae.encode(G(g["x_crop"], dev)).cpu(), g["z_crop"]) < TOL


def test_vae_encode_folded_route(dev):
    """Round 5, encoder (bf16x3, two conv blocks, pooling (4, 8, 8)): the first convolution on the halo-tile kernel with two taps per
    k-step (ABI 7 conv0_pk_w3), its output straight into conv 1's operand image, GroupNorm 0 folded into conv 1's per-sample weights
    and border table, conv 1's epilogue -> pooling partial sums -> GroupNorm 1 + AvgPool3d + to_lat (vae_video3d.py:164-189): no fp32
    activation is written.  Against the golden fixture (also its cropped input) and the route with fp32 activations between the kernels;
    f16x2 takes the pooling part only."""
    import warnings
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import _lib as L
    g = load_golden("g12_vae_encode.npz")
    for mode in ("bf16x3", "f16x2"):
        outs = {}
        with tuned("vae_fold"):
            for fold in (0, 1):
                tune("vae_fold", fold)
                vae = A.VideoVAE.from_config({"latent": {"channels": 8, "t_down": 4, "s_down": 8}}).eval()
                vae.load_state_dict(split_weights(g)["w"], strict=False)
                vae = vae.to(dev)
                vae.matmul = mode
                L.prof_enable(True)
                z = vae.encode(G(g["x"], dev)).cpu()
                torch.cuda.synchronize()
                L.prof_enable(False)
                used = {k for k, v in L.prof_report().items() if v[0] > 0}
                want = {"rgb_lat16_kernel", "conv3d_k3_bf16x3_kernel<6, 0, 1>", "conv3d_k3_bf16x3_kernel<6, 4, 3>", "pool_tolat_from_partials_kernel"} \
                    if mode == "bf16x3" else {"conv3d_k3_bf16x3_kernel<3, 4, 3>", "pool_tolat_from_partials_kernel"}
                assert (want <= used) == bool(fold), used
                assert ("gn_pool_tolat_kernel" in used) == (not fold), used
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    outs[fold] = (z, vae.encode(G(g["x_crop"], dev)).cpu())
            assert rel_err(outs[1][0], g["z"]) < TOL and rel_err(outs[1][1], g["z_crop"]) < TOL
            assert rel_err(outs[1][0], outs[0][0]) < 2e-5 and rel_err(outs[1][1], outs[0][1]) < 2e-5


def test_full_step_v2a_bf16x3(dev, full):
    """Video -> audio direction on the bf16x3 path: 37 target + 384 prompt tokens at 256x256 (the prompt is the long part, the
    target rows come first, the audio head stays on fp32 MFMA), B=10 -> 8,420 rows; oracle on the first two samples."""
    ws, _ = full
    core, head, av, aa = modules(dev, ws, 8)
    g = torch.Generator().manual_seed(78)
    B = 10
    z_v = torch.randn(B, 8, 12, 32, 32, generator=g)
    z_a = torch.randn(B, 8, 150, generator=g)
    abar = R.alpha_bar_table(R.beta_table(1000))
    tn = torch.tensor([982, 19] * 5)
    tp = torch.tensor([966, -1] * 5)
    ref = R.denoise_step_v2a(z_a[:2], z_v[:2], tn[:2], tp[:2], abar, adapt_v=ws["adapt_v"], adapt_a=ws["adapt_a"], core=ws["core"],
                             head=ws["head"], n_layers=8, n_heads=8, guidance=3.0)
    eng = engine((core, head, av, aa), "audio", tuple(z_a.shape), 384, alpha_bar=abar, guidance=3.0, matmul="bf16x3")
    eng.set_prompt(z_v.to(dev))
    out = eng.step(z_a.to(dev), tn.to(dev), tp.to(dev))
    assert rel_err(out[:2].cpu(), ref) < TOL
    f32 = engine((modules(dev, ws, 8)[0], head, av, aa), "audio", tuple(z_a.shape), 384, alpha_bar=abar, guidance=3.0, matmul="f32")
    f32.set_prompt(z_v.to(dev))
    o32 = f32.step(z_a.to(dev), tn.to(dev), tp.to(dev))
    assert not torch.equal(out, o32) and rel_err(out.cpu(), o32.cpu()) < 2e-5


@pytest.mark.parametrize("B,C,T,H,W,eta", [(3, 8, 12, 32, 32, 0.0), (2, 8, 12, 64, 64, 0.0), (2, 8, 12, 16, 16, 0.5), (5, 8, 4, 8, 32, 0.0),
                                            (2, 8, 4, 8, 8, 0.0)])
def test_cfg_unpatch_ddim_row_form_is_bit_identical(dev, B, C, T, H, W, eta):
    """Round 5: the fused CFG + un-patch + DDIM kernel moves whole token rows in and whole 128-byte latent lines out through an LDS
    transpose (avd_tune_set "cfg_rows" 1, default) instead of one 16-byte gather per lane: the same arithmetic per element — results
    equal bit for bit (W = 32 / 64: eight tokens per line; W = 16: four; W = 8 falls back to the gather form), and both match the oracle."""
    from multimodal_diffusion_amd import _lib as L
    g = torch.Generator().manual_seed(B * 100 + W)
    Nv = (T // 2) * (H // 4) * (W // 4)
    eps2 = torch.randn(2 * B, Nv, C * 2 * 4 * 4, generator=g)
    z = torch.randn(B, C, T, H, W, generator=g)
    noise = torch.randn(B, C, T, H, W, generator=g) if eta > 0 else None
    tn = torch.tensor([982, 500, 16, 999, 3][:B])
    tp = torch.tensor([966, 480, -1, 979, -1][:B])
    abar = R.alpha_bar_table(R.beta_table(1000))
    outs = {}
    d_eps, d_z, d_tn, d_tp, d_ab = eps2.to(dev), z.to(dev), tn.to(dev), tp.to(dev), abar.to(dev)     # (kept alive across the launches)
    d_noise = None if noise is None else noise.to(dev)
    for rows in (0, 1):
        with tuned(cfg_rows=rows):
            out = torch.empty(B, C, T, H, W, device=dev)
            L.check(L.lib().avd_cfg_unpatch_ddim_f32(d_eps.data_ptr(), d_z.data_ptr(), d_tn.data_ptr(), d_tp.data_ptr(), d_ab.data_ptr(), 1000, 3.5,
                                                     eta, L.ptr(d_noise), out.data_ptr(), B, C, T, H, W, 2, 4, 4, L.stream_ptr(dev)))
            torch.cuda.synchronize()
            outs[rows] = out.cpu()
    assert torch.equal(outs[0], outs[1])
    e = eps2[B:] + 3.5 * (eps2[:B] - eps2[B:])
    if eta == 0:
        ref = R.ddim_update(z.double(), tn, tp, R.tube_unpatch(e.double(), C, T, H, W, 2, 4, 4), abar.double())
        assert rel_err(outs[1], ref) < 1e-5


# ------------------------------------------------------------------------------------------------- round-2 coverage
def _sample_rows(M, g):
    idx = torch.cat([torch.arange(0, min(M, 192)), torch.arange(max(0, M - 192), M),
                     torch.randint(0, M, (384,), generator=g)]).unique()
    return idx


@pytest.mark.parametrize("tile", [0, 1, 2])
@pytest.mark.parametrize("M,N,K", [(16385, 512, 512), (26944, 1536, 512), (20011, 2048, 512), (16500, 512, 2048)])
@pytest.mark.parametrize("mode", ["plain", "gelu", "res"])
def test_gemm_dma_templates_direct(dev, tile, M, N, K, mode):
    """Each LDS-DMA tile template (0: 128x128, 1: 128x64, 2: 64x64) forced in turn at full-batch row counts with ragged M,
    every epilogue, against fp64 on a row sample that includes the first and the ragged last row blocks."""
    from multimodal_diffusion_amd import functional as Fn, _lib as L
    g = torch.Generator().manual_seed(M + N + K + tile)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    b = torch.randn(N, generator=g)
    r = torch.randn(M, N, generator=g)
    idx = _sample_rows(M, g)
    ref = R.linear(x[idx].double(), w.double(), b.double())
    if mode == "gelu":
        ref = R.gelu_erf(ref)
    if mode == "res":
        ref = ref + r[idx].double()
    with tuned(gemm_tile=tile):
        y = Fn.linear(x.to(dev), w.to(dev), b.to(dev), act=L.ACT_GELU if mode == "gelu" else L.ACT_NONE,
                      residual=r.to(dev) if mode == "res" else None)
    assert torch.isfinite(y).all()
    assert rel_err(y.cpu()[idx], ref) < 2e-5


@pytest.mark.parametrize("tile", [0, 1, 2])
@pytest.mark.parametrize("M", [16385, 26944])
def test_gemm_rmsfold_epilogue_direct(dev, tile, M):
    """The folded-RMSNorm epilogues stand-alone: a residual GEMM that emits per-row sums of squares (ss_out), then the
    scale-carrying GEMM that consumes them (ss_in) — against RMSNorm -> Linear in fp64 (mmdt.py:39-42, 77-83)."""
    from multimodal_diffusion_amd import functional as Fn, _lib as L
    d, hid = 512, 2048
    g = torch.Generator().manual_seed(M + tile)
    a = torch.randn(M, d, generator=g)
    x0 = torch.randn(M, d, generator=g) * torch.exp(torch.randn(M, 1, generator=g))       # rows of very different norms
    x0[7] = 0.0                                                                           # all-zero row: eps carries it
    w0 = torch.randn(d, d, generator=g) / math.sqrt(d)
    b0 = torch.randn(d, generator=g) * 0.1
    scale = 1.0 + 0.1 * torch.randn(d, generator=g)
    w1 = torch.randn(hid, d, generator=g) / math.sqrt(d)
    b1 = torch.randn(hid, generator=g) * 0.1
    idx = _sample_rows(M, g)
    with tuned(gemm_tile=tile):
        x1, ss = Fn.linear_rmsfold(a.to(dev), w0.to(dev), b0.to(dev), residual=x0.to(dev), want_ss=True)
        y, _ = Fn.linear_rmsfold(x1, (w1 * scale[None, :]).to(dev), b1.to(dev), act=L.ACT_GELU, ss_in=ss, eps=1e-6)
        # the one-column table form (first block: rowss kernel)
        ss1 = (x1 * x1).sum(-1, keepdim=True).contiguous()
        y1, _ = Fn.linear_rmsfold(x1, (w1 * scale[None, :]).to(dev), b1.to(dev), act=L.ACT_GELU, ss_in=ss1, eps=1e-6)
    x1_ref = x0[idx].double() + R.linear(a[idx].double(), w0.double(), b0.double())
    assert rel_err(x1.cpu()[idx], x1_ref) < 2e-5
    chunks = x1.cpu().double().view(M, d // 32, 32).pow(2).sum(-1)
    assert rel_err(ss.cpu(), chunks) < 1e-5
    # reference on the device's own x1 so only the folded GEMM is under test
    h = R.rmsnorm(x1.cpu()[idx].double(), scale.double(), 1e-6)
    ref = R.gelu_erf(R.linear(h, w1.double(), b1.double()))
    assert rel_err(y.cpu()[idx], ref) < 2e-5
    assert rel_err(y1.cpu()[idx], ref) < 2e-5


@pytest.mark.parametrize("B,N,H", [(1, 1573, 8), (2, 1600, 2), (1, 1537, 4)])
def test_attention_long(dev, B, N, H):
    """BASELINE C5 geometry (512x512: 1536 + 37 = 1573 tokens, 25 key tiles) on the default fp32 kernel."""
    from multimodal_diffusion_amd import functional as Fn
    g = torch.Generator().manual_seed(B * 1000 + N)
    d = 64 * H
    qkv = torch.randn(B, N, 3 * d, generator=g) * 1.5
    q, k, v = (qkv.double().view(B, N, 3, H, 64)[:, :, i].transpose(1, 2) for i in range(3))
    ref = (torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1) @ v).transpose(1, 2).reshape(B, N, d)
    assert rel_err(Fn.attention(qkv.to(dev), H).cpu(), ref) < 2e-5
    nq = N - 37
    part = Fn.attention(qkv.to(dev), H, n_query=nq)
    assert rel_err(part[:, :nq].cpu(), ref[:, :nq]) < 2e-5 and torch.count_nonzero(part[:, nq:]) == 0


def _one_step(dev, mods, ws, size, B, n_ref, matmul="f32", seed=None):
    core, head, av, aa = mods
    g = torch.Generator().manual_seed(size if seed is None else seed)
    z_v = torch.randn(B, 8, 12, size // 8, size // 8, generator=g)
    z_a = torch.randn(B, 8, 150, generator=g)
    abar = R.alpha_bar_table(R.beta_table(1000))
    tn = torch.tensor(([982, 500, 16, 999] * B)[:B])
    tp = torch.tensor(([966, 480, -1, 979] * B)[:B])
    ref = R.denoise_step_a2v(z_v[:n_ref], z_a[:n_ref], tn[:n_ref], tp[:n_ref], abar, adapt_v=ws["adapt_v"], adapt_a=ws["adapt_a"],
                             core=ws["core"], head=ws["head"], n_layers=8, n_heads=8, guidance=3.5)
    eng = engine((core, head, av, aa), "video", tuple(z_v.shape), 37, alpha_bar=abar, guidance=3.5, matmul=matmul)
    eng.set_prompt(z_a.to(dev))
    return eng.step(z_v.to(dev), tn.to(dev), tp.to(dev)).cpu(), ref


def test_full_step_f32_512(dev, full):
    """BASELINE C5 geometry on the DEFAULT fp32 path: 512x512, N = 1573, B = 4 (2B*N = 12,584 rows: the 128-row tiles),
    sample 0 against the CPU oracle."""
    ws, mods = full
    out, ref = _one_step(dev, mods, ws, 512, 4, 1)
    assert rel_err(out[:1], ref) < TOL


@pytest.mark.parametrize("matmul", ["bf16x3", "f16x2", "bf16x3_strict"])
def test_full_step_c3_batch32_split_modes(dev, full, matmul):
    """The bench's workload exactly — BASELINE C3: 256x256, 384 + 37 tokens, batch 32 (2B*N = 26,944 rows: the 8-wave 256x256 and the
    4-wave 256x128 split GEMMs, folded norms, four rounds of attention blocks) — in the headline mode (bf16x3), its strict variant and
    the speed mode (f16x2), one CFG step against the CPU oracle on samples from the start, the middle and the end of the batch
    (only bench.py checked B = 32; smaller batches take other tile counts and super-tile shapes)."""
    ws, mods = full
    core, head, av, aa = mods
    B, idx = 32, [0, 17, 31]
    g = torch.Generator().manual_seed(2560)
    z_v = torch.randn(B, 8, 12, 32, 32, generator=g)
    z_a = torch.randn(B, 8, 150, generator=g)
    abar = R.alpha_bar_table(R.beta_table(1000))
    tn = torch.tensor(([982, 500, 16, 999] * B)[:B])
    tp = torch.tensor(([966, 480, -1, 979] * B)[:B])
    eng = engine((core, head, av, aa), "video", tuple(z_v.shape), 37, alpha_bar=abar, guidance=3.5, matmul=matmul)
    eng.set_prompt(z_a.to(dev))
    out = eng.step(z_v.to(dev), tn.to(dev), tp.to(dev)).cpu()
    ref = R.denoise_step_a2v(z_v[idx], z_a[idx], tn[idx], tp[idx], abar, adapt_v=ws["adapt_v"], adapt_a=ws["adapt_a"], core=ws["core"],
                             head=ws["head"], n_layers=8, n_heads=8, guidance=3.5)
    err = rel_err(out[idx], ref)
    print(f"C3 batch 32, {matmul}: rel err vs CPU oracle {err:.3e}")
    assert torch.isfinite(out).all() and err < TOL


def test_full_step_c2_batch32(dev, full):
    """BASELINE C2 shape at its real batch: 64x64, N = 61, B = 32 (3,904 rows -> the 64x64 tiles), fp32; first two samples."""
    ws, mods = full
    out, ref = _one_step(dev, mods, ws, 64, 32, 2)
    assert rel_err(out[:2], ref) < TOL


def test_vae_decode_256_vs_oracle(dev):
    """Row a9 at the headline geometry: one sample [1,8,12,32,32] -> [1,3,48,256,256] against the fp32 CPU oracle."""
    import multimodal_diffusion_amd as A
    W = R.synth_vae_decoder(seed=5, n_blocks=2)
    vae = A.VideoVAE(A.VideoVAEConfig()).eval()
    vae.load_state_dict(W, strict=False)
    z = torch.randn(1, 8, 12, 32, 32, generator=torch.Generator().manual_seed(6))
    ref = R.vae_decode(z, W, n_blocks=2)
    x = vae.to(dev).decode(z.to(dev)).cpu()
    assert x.shape == (1, 3, 48, 256, 256)
    assert rel_err(x, ref) < TOL


def test_vae_decode_512_routes_agree(dev):
    """The C5 geometry's decode (one sample [1,8,12,64,64] -> [1,3,48,512,512]: 12.6 M voxels, 4.8 GB operand image): the default
    route (composed + packed first conv, folded GroupNorm, to_img from partial sums) against the three-pass route with fp32 activations
    between the kernels — same operator up to fp32 rounding, index arithmetic included at four times the headline volume."""
    import multimodal_diffusion_amd as A
    W = R.synth_vae_decoder(seed=9, n_blocks=2)
    z = torch.randn(1, 8, 12, 64, 64, generator=torch.Generator().manual_seed(10)).to(dev)
    outs = {}
    with tuned("vae_fold"):
        for route in ("default", "three passes"):
            tune("vae_fold", 1 if route == "default" else 0)
            vae = A.VideoVAE(A.VideoVAEConfig()).eval()
            vae.load_state_dict(W, strict=False)
            vae.matmul, vae.lat_composed = "bf16x3", route == "default"
            outs[route] = vae.to(dev).decode(z)
            del vae
    assert outs["default"].shape == (1, 3, 48, 512, 512) and bool(torch.isfinite(outs["default"]).all())
    assert float((outs["default"] - outs["three passes"]).abs().max()) < 2e-5


def test_add_mode_step_golden(dev, small_model):
    """next-4 pinned: trainer-style embedding (train/trainer.py:36-49) against the G15 fixture made by the reference's own
    helper definitions."""
    import multimodal_diffusion_amd as A
    _, W, meta = small_model
    core, head, _, _ = _small_modules(dev, W, meta)
    g = load_golden("g15_add_mode_step.npz")
    Wa = split_weights(g)
    av, aa = A.LinearAdapter(256, meta["d"]), A.LinearAdapter(32, meta["d"])
    av.load_state_dict(Wa["adapt_v"], strict=True)
    aa.load_state_dict(Wa["adapt_a"], strict=True)
    z_v = G(g["z_v"], dev)
    eng = A.DenoiseEngine(adapt_v=av.to(dev), adapt_a=aa.to(dev), core=core, head=head, tstep_dim=meta["tdim"], target="video",
                          latent_shape=tuple(z_v.shape), prompt_tokens=5, alpha_bar=T(g["abar"]), guidance=float(g["guidance"]),
                          temb_mode="add")
    eng.set_prompt(G(g["z_a"], dev))
    zn = eng.step(z_v, G(g["t_now"], dev), G(g["t_prev"], dev))
    e2 = eng.eps_tokens()
    B = z_v.shape[0]
    assert rel_err(e2[:B].cpu(), g["eps_cond"]) < TOL and rel_err(e2[B:].cpu(), g["eps_null"]) < TOL
    assert rel_err(zn.cpu(), g["z_next"]) < TOL


@pytest.mark.parametrize("matmul", ["f32", "bf16x3"])
def test_engine_follows_weight_updates(dev, full, matmul):
    """Weights loaded AFTER the engine was built (load_state_dict writes in place): the next step must use the new weights
    everywhere, including the derived norm-folded / split3 copies — checked against the oracle with the new weights."""
    ws, _ = full
    core, head, av, aa = modules(dev, ws, 8)
    B = 16 if matmul == "bf16x3" else 2           # 2B*N = 13,472 rows takes the bf16x3 kernels
    g = torch.Generator().manual_seed(31)
    z_v = torch.randn(B, 8, 12, 32, 32, generator=g)
    z_a = torch.randn(B, 8, 150, generator=g)
    abar = R.alpha_bar_table(R.beta_table(1000))
    tn, tp = torch.full((B,), 500), torch.full((B,), 480)
    eng = engine((core, head, av, aa), "video", tuple(z_v.shape), 37, alpha_bar=abar, guidance=3.5, matmul=matmul)
    eng.set_prompt(z_a.to(dev))
    before = eng.step(z_v.to(dev), tn.to(dev), tp.to(dev)).cpu()
    ws2 = R.synth_weights(seed=9)
    core.load_state_dict(ws2["core"])
    head.load_state_dict(ws2["head"])
    av.load_state_dict(ws2["adapt_v"])
    aa.load_state_dict(ws2["adapt_a"])
    after = eng.step(z_v.to(dev), tn.to(dev), tp.to(dev)).cpu()
    ref = R.denoise_step_a2v(z_v[:2], z_a[:2], tn[:2], tp[:2], abar, adapt_v=ws2["adapt_v"], adapt_a=ws2["adapt_a"],
                             core=ws2["core"], head=ws2["head"], n_layers=8, n_heads=8, guidance=3.5)
    assert not torch.equal(before, after)
    assert rel_err(after[:2], ref) < TOL


@pytest.mark.parametrize("matmul", ["f32", "bf16x3", "f16x2", "auto"])
def test_class_default_width_golden(dev, matmul):
    """VERDICT r3 missing 4: the reference's CLASS-DEFAULT geometry — MMDiT(d_model=1024, n_heads=16) (mmdt.py:125-126; two layers) on
    16 x 421 tokens (6,736 rows: the split kernels engage) and MultiModalNoiseHead at d = 1024 with the reference shape test's token
    counts (tests/test_shapes.py:86-107: Nv = 96, Na = 37; batch 64 = 6,144 video rows) — against fixture g18 (the reference's own
    modules on seeded-recipe weights) and against the oracle on whole samples.  Widths other than mvp.yaml's take other kernel
    variants: N = 1024 residual epilogues (four column blocks, 16 sum-of-squares chunks per row), K = 4096 fc2, 16-head q|k|v
    images, no row-owner norm epilogue in f16x2 (that one needs N == 512: separate norm kernels run instead)."""
    import multimodal_diffusion_amd as A
    g = load_golden("g18_class_default_width.npz")
    meta = json.loads(str(g["meta"]))
    ws = R.synth_weights(seed=meta["seed_weights"], d=1024, n_layers=2)
    gen = torch.Generator().manual_seed(meta["seed_inputs"])
    x = torch.randn(16, 421, 1024, generator=gen)
    hv = torch.randn(64, 96, 1024, generator=gen)
    ha = torch.randn(64, 37, 1024, generator=gen)
    core = A.MMDiT(d_model=1024, n_layers=2, n_heads=16).eval()
    core.load_state_dict(ws["core"], strict=True)
    head = A.MultiModalNoiseHead(input_dims={"video": 1024, "audio": 1024}, output_dims={"video": 256, "audio": 32}, hidden_dim=512,
                                 num_shared_layers=2, num_modality_specific_layers=1, dropout=0.1, activation="gelu").eval()
    head.load_state_dict(ws["head"], strict=True)
    core, head = core.to(dev), head.to(dev)
    core.matmul = head.matmul = matmul
    y = core(x.to(dev)).cpu()
    e_gold = max(rel_err(y[0, ::8], g["core_first"]), rel_err(y[-1, ::8], g["core_last"]))
    e_orc = rel_err(y[[0, 7]], R.mmdit_forward(x[[0, 7]], ws["core"], 2, 16))
    out = head({"video": hv.to(dev), "audio": ha.to(dev)})
    ov, oa = out["video"].cpu(), out["audio"].cpu()
    assert ov.shape == (64, 96, 256) and oa.shape == (64, 37, 32)
    e_head = max(rel_err(ov[0], g["head_video_first"]), rel_err(ov[-1], g["head_video_last"]), rel_err(oa[0], g["head_audio_first"]))
    e_head_orc = rel_err(ov[[5, 40]], R.noise_head(hv[[5, 40]], ws["head"], "video"))
    print(f"d_model 1024, {matmul}: core vs golden {e_gold:.2e}, vs oracle {e_orc:.2e}; head vs golden {e_head:.2e}, vs oracle {e_head_orc:.2e}")
    assert torch.isfinite(y).all() and max(e_gold, e_orc, e_head, e_head_orc) < TOL
    # the reference shape test's own call (B = 2: 192 + 74 rows, fp32 kernels whatever the mode)
    small = head({"video": hv[:2].to(dev), "audio": ha[:2].to(dev)})
    assert rel_err(small["video"].cpu(), R.noise_head(hv[:2], ws["head"], "video")) < TOL
    assert rel_err(small["audio"].cpu(), R.noise_head(ha[:2], ws["head"], "audio")) < TOL


@pytest.mark.parametrize("d,H,hid", [(768, 12, 3072), (256, 4, 1024), (384, 6, 1536), (512, 8, 1024)])
def test_other_widths_fall_back_or_run(dev, d, H, hid):
    """Widths the split kernels cover (every projection width a multiple of 256: d = 768, 256) run them; widths they refuse (d = 384:
    3 d = 1,152 is not) take the fp32 MFMA kernels without a word — both against the oracle in the headline mode at a row count
    past the split threshold, so whichever path is taken is the one being checked."""
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import _lib as L
    ws = R.synth_weights(seed=d, d=d, n_layers=2, mlp_ratio=hid / d)
    core = A.MMDiT(d_model=d, n_layers=2, n_heads=H, mlp_ratio=hid / d).eval()
    core.load_state_dict(ws["core"], strict=True)
    core = core.to(dev)
    x = torch.randn(16, 421, d, generator=torch.Generator().manual_seed(d + 1))
    ref = R.mmdit_forward(x[:2], ws["core"], 2, H)
    for mode in ("bf16x3", "f16x2", "f32"):
        core.matmul = mode
        core(x.to(dev))
        L.prof_enable(True)
        y = core(x.to(dev)).cpu()
        torch.cuda.synchronize()
        L.prof_enable(False)
        used = {k for k, v in L.prof_report().items() if v[0] > 0}
        split = any(k.startswith("gemm_bf16x3") for k in used)
        assert split == (mode != "f32" and d % 256 == 0 and hid % 256 == 0), (d, mode, used)
        assert rel_err(y[:2], ref) < TOL, (d, mode)


@pytest.mark.parametrize("matmul", ["bf16x3", "f16x2", "auto"])
def test_full_step_shipped_geometry_batch32(dev, full, matmul):
    """the reference's SHIPPED geometry (configs/mvp.yaml:32 — 128 x 128 video: 96 + 37 tokens) at batch 32:
    2B*N = 8,512 rows, just above the split kernels' 6,144-row threshold, where every projection takes the 256 x 128 blocks.  One CFG
    step against the CPU oracle (not against the fp32 mode) on samples from the start, middle and end of the batch."""
    ws, mods = full
    core, head, av, aa = mods
    B, idx = 32, [0, 13, 31]
    g = torch.Generator().manual_seed(1280)
    z_v = torch.randn(B, 8, 12, 16, 16, generator=g)
    z_a = torch.randn(B, 8, 150, generator=g)
    abar = R.alpha_bar_table(R.beta_table(1000))
    tn = torch.tensor(([982, 500, 16, 999] * B)[:B])
    tp = torch.tensor(([966, 480, -1, 979] * B)[:B])
    eng = engine((core, head, av, aa), "video", tuple(z_v.shape), 37, alpha_bar=abar, guidance=3.5, matmul=matmul)
    eng.set_prompt(z_a.to(dev))
    out = eng.step(z_v.to(dev), tn.to(dev), tp.to(dev)).cpu()
    ref = R.denoise_step_a2v(z_v[idx], z_a[idx], tn[idx], tp[idx], abar, adapt_v=ws["adapt_v"], adapt_a=ws["adapt_a"], core=ws["core"],
                             head=ws["head"], n_layers=8, n_heads=8, guidance=3.5)
    err = rel_err(out[idx], ref)
    print(f"128x128 batch 32, {matmul}: rel err vs CPU oracle {err:.3e}")
    assert torch.isfinite(out).all() and err < TOL


@pytest.mark.parametrize("B,N,nq", [(16, 421, 384), (3, 2100, 2048), (20, 421, 1)])
def test_last_block_runs_on_the_output_window_only(dev, full, B, N, nq):
    """VERDICT r3 missing 6: with the caller's row window at row 0 (the engine passes the target rows) the last block's attention
    writes its rows compactly and out_proj / fc1 / fc2 / the final norm run on B * n_out_rows rows (residual read through a row map).
    Every row's arithmetic is unchanged, so the window of the result equals the full-window forward BIT FOR BIT, in the headline
    mode, at the bench's row ratio (384 of 421), at a ragged multi-block shape and at a one-row window; `core_trim` 0 (the
    untrimmed last block) agrees as well."""
    import ctypes as C
    from multimodal_diffusion_amd import _lib as L
    ws, mods = full
    core = mods[0]
    prev = core.matmul
    core.matmul = "bf16x3"
    try:
        x = torch.randn(B, N, 512, generator=torch.Generator().manual_seed(B + N)).to(dev)
        cw, keep = core.weight_table()
        wsb = torch.empty(L.lib().avd_core_workspace_bytes(C.byref(cw), B, N), dtype=torch.uint8, device=dev)

        def fwd(rows, trim):
            with tuned(core_trim=trim):
                y = torch.zeros_like(x)
                L.check(L.lib().avd_core_forward_f32(C.byref(cw), x.data_ptr(), y.data_ptr(), B, N, 0, rows, None, wsb.data_ptr(), wsb.numel(),
                                                     L.stream_ptr(dev)))
                torch.cuda.synchronize()
                return y
        whole = fwd(N, 1)
        assert torch.isfinite(whole).all()
        assert rel_err(whole[:1].cpu(), R.mmdit_forward(x[:1].cpu(), ws["core"], 8, 8)) < TOL
        for trim in (1, 0):
            part = fwd(nq, trim)
            assert torch.equal(part[:, :nq], whole[:, :nq]), (trim, float((part[:, :nq] - whole[:, :nq]).abs().max()))
        del keep
    finally:
        core.matmul = prev


@pytest.mark.parametrize("B", [8, 32])
def test_fused_mlp_matches_two_launches(dev, full, B):
    """fc1 -> GELU -> fc2 of a block as ONE launch (csrc/mlp_bf16x3.hip, avd_tune_set "mlp_fused" 1; the hidden
    chunk stays in LDS, the fc2 accumulators in AGPRs).  Same operands, same six product terms in the same order: a whole CFG step at the
    bench's geometry is BIT-IDENTICAL to the two-launch path — B = 8 (6,736 rows; without the last-block trim as well, whose fused
    call writes the fp32 stream only) and the bench's B = 32.  (Until split8 switched contraction off, the compiler fused the GELU's
    last multiply into the split's `a - h` in this kernel and not in the fc1 kernel, and the two disagreed by 1 ulp: avd_common.h.)"""
    from multimodal_diffusion_amd import _lib as L
    ws, mods = full
    core, head, av, aa = mods
    g = torch.Generator().manual_seed(900 + B)
    z_v = torch.randn(B, 8, 12, 32, 32, generator=g)
    z_a = torch.randn(B, 8, 150, generator=g)
    abar = R.alpha_bar_table(R.beta_table(1000))
    tn = torch.tensor(([982, 500, 16, 999] * B)[:B])
    tp = torch.tensor(([966, 480, -1, 979] * B)[:B])
    outs = {}
    with tuned("mlp_fused", "core_trim", s3_splitk=0):        # (split-K of fc2 and the fused launch exclude each other: keep both arms on whole-K sums)
        for fused, trim in ((0, 1), (1, 1), (1, 0)):
            tune("mlp_fused", fused)
            tune("core_trim", trim)
            eng = engine((core, head, av, aa), "video", tuple(z_v.shape), 37, alpha_bar=abar, guidance=3.5, matmul="bf16x3")
            eng.set_prompt(z_a.to(dev))
            eng.step(z_v.to(dev), tn.to(dev), tp.to(dev))
            L.prof_enable(True)
            outs[fused, trim] = eng.step(z_v.to(dev), tn.to(dev), tp.to(dev)).cpu()
            torch.cuda.synchronize()
            L.prof_enable(False)
            rep = L.prof_report()
            assert (rep.get("mlp_bf16x3_kernel", (0,))[0] > 0) == bool(fused), rep.keys()
            if fused:
                print(f"fused MLP, B={B}, trim={trim}: {1e3 * rep['mlp_bf16x3_kernel'][1] / rep['mlp_bf16x3_kernel'][0]:.1f} us per launch")
    assert torch.isfinite(outs[0, 1]).all() and torch.isfinite(outs[1, 1]).all()
    d1, d0 = rel_err(outs[1, 1], outs[0, 1]), rel_err(outs[1, 0], outs[0, 1])
    assert torch.equal(outs[1, 0], outs[1, 1])                 # the fused path with and without the trimmed last block: bit-identical
    ref = R.denoise_step_a2v(z_v[:1], z_a[:1], tn[:1], tp[:1], abar, adapt_v=ws["adapt_v"], adapt_a=ws["adapt_a"], core=ws["core"],
                             head=ws["head"], n_layers=8, n_heads=8, guidance=3.5)
    e1, e0 = rel_err(outs[1, 1][:1], ref), rel_err(outs[0, 1][:1], ref)
    print(f"fused MLP, B={B}: vs two launches {d1:.2e}; vs CPU oracle {e1:.3e} (two launches: {e0:.3e})")
    assert torch.equal(outs[1, 1], outs[0, 1]), (d1, d0)
    assert e1 < TOL


def test_f32_splitk_tiny_batch(dev, full):
    """BASELINE C1 geometry (32x32, batch 4: 2B*N = 344 rows): the fp32 fc2 launch is 48 blocks of 64 x 64 that each walk K = 2,048;
    avd_tune_set "gemm_splitk" (default 4) cuts K into four slices (blockIdx.y) whose partial sums a reduction kernel adds in slice
    order before bias and residual, writing the stream and the rows' sums of squares for the next folded norm.  Against the one-launch
    path only the summation order differs; both sit at the parity tolerance from the CPU oracle; the split path is repeatable bit for
    bit."""
    from multimodal_diffusion_amd import _lib as L
    ws, mods = full
    outs = []
    with tuned("gemm_splitk"):
        for ns in (4, 0, 4):
            tune("gemm_splitk", ns)
            L.prof_enable(True)
            out, ref = _one_step(dev, mods, ws, 32, 4, 4, matmul="f32")
            torch.cuda.synchronize()
            L.prof_enable(False)
            ran = L.prof_report().get("splitk_reduce_f32_kernel", (0,))[0] > 0
            assert ran == (ns > 0), (ns, ran)
            outs.append(out)
    assert torch.equal(outs[0], outs[2]) and not torch.equal(outs[0], outs[1])
    d, e4, e0 = rel_err(outs[0], outs[1]), rel_err(outs[0], ref), rel_err(outs[1], ref)
    print(f"fp32 split-K fc2 at C1: vs one launch {d:.2e}; vs CPU oracle {e4:.3e} (one launch {e0:.3e})")
    assert d < 1e-5 and e4 < TOL and e0 < TOL          # (measured 3.1e-6: the step amplifies the last bits of eps)


def test_default_mode_is_the_headline_mode(dev):
    """modules built through `build_components` from an mvp.yaml-shaped config with NO runtime override run the
    bench's headline kernels at the bench's size (matmul "auto" -> bf16x3 where the split kernels engage) and the norm-folded fp32
    MFMA kernels at a small batch; the auto engine's step is bit-identical to an explicit bf16x3 engine's (same kernels)."""
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import _lib as L
    cfg = {"tokenizer": {"width": 512}, "embeddings": {"timestep_dim": 256},
           "model": {"core": dict(d_model=512, n_layers=8, n_heads=8, mlp_ratio=4.0, dropout=0.1, attn_dropout=0.0, norm="rmsnorm",
                                  rope=False, token_dropout=0.0),
                     "heads": {"video": dict(out_dim=256, hidden_dim=512, num_layers=2, dropout=0.1, activation="gelu"),
                               "audio": dict(out_dim=32, hidden_dim=512, num_layers=2, dropout=0.1, activation="gelu")}}}
    torch.manual_seed(0)
    _, _, av, aa, core, head, tdim = A.build_components(cfg, dev)
    assert core.matmul == "auto" and head.matmul == "auto" and A.MMDiT().matmul == "auto"
    abar = R.alpha_bar_table(R.beta_table(1000))
    g = torch.Generator().manual_seed(4)

    def tags(B, hw, matmul=None):
        z = torch.randn(B, 8, 12, hw, hw, generator=g).to(dev)
        za = torch.randn(B, 8, 150, generator=g).to(dev)
        eng = engine((core, head, av, aa), "video", tuple(z.shape), 37, alpha_bar=abar, guidance=3.5, tstep_dim=tdim, matmul=matmul)
        eng.set_prompt(za)
        tn, tp = torch.full((B,), 500, device=dev), torch.full((B,), 480, device=dev)
        eng.step(z, tn, tp)
        torch.cuda.synchronize()
        L.prof_enable(True)
        out = eng.step(z, tn, tp)
        torch.cuda.synchronize()
        L.prof_enable(False)
        return {k for k, v in L.prof_report().items() if v[0] > 0}, out, (z, za, tn, tp)

    big, out_auto, (z, za, tn, tp) = tags(32, 32)                      # C3: 2 x 32 x 421 = 26,944 rows
    assert any(k.startswith(("gemm_bf16x3", "mlp_bf16x3")) for k in big) and any(k.startswith("attn_bf16x3") for k in big), big
    assert not any(k.startswith("gemm_f32_dma") for k in big), big      # no block projection on the fp32 MFMA kernels
    eng3 = engine((core, head, av, aa), "video", tuple(z.shape), 37, alpha_bar=abar, guidance=3.5, tstep_dim=tdim, matmul="bf16x3")
    eng3.set_prompt(za)
    assert torch.equal(eng3.step(z, tn, tp), out_auto)
    small, out_small, _ = tags(2, 8)                                    # 2 x 2 x 61 rows: below the split kernels' threshold
    assert not any(k.startswith(("gemm_bf16x3", "attn_bf16x3")) for k in small), small
    assert any(k.startswith("gemm_f32") for k in small), small
    assert torch.isfinite(out_small).all()


@pytest.mark.parametrize("N,K", [(512, 512), (256, 64), (512, 2048)])
def test_split_gemm_short_blocks_ragged_rows(dev, N, K):
    """The short-block / four-stage-ring variants of the four-wave split GEMM at the C ABI (avd_gemm_bf16x3_f32), at row counts that do
    not fit anything: 1 row, one row either side of a 32-row piece and of a 160-row block, a prime, a 128-row group plus one — fewer rows
    than one block, last blocks that start in the image's last 128-row group, blocks whose upper waves own no valid row.  For every
    epilogue the C ABI reaches (fp32 out with bias: the register bias epilogue; + residual: the residual epilogue without an image;
    GELU -> operand image) every block size (avd_tune_set "s3_rt4" 2 .. 8) on either ring ("s3_deep4") returns the bits of the 256-row
    blocks, and those are within the fp32 FMA chain's bound of the fp64 product."""
    from multimodal_diffusion_amd import functional as Fn, _lib as L
    g = torch.Generator().manual_seed(N + K)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    w3 = Fn.split3(w.to(dev))
    for M in (1, 31, 33, 159, 161, 257, 1009, 2049):
        x = torch.randn(M, K, generator=g)
        r = torch.randn(M, N, generator=g)
        x3 = Fn.split3(x.to(dev))
        ref = x.double() @ w.double().t() + b.double()
        outs = {}
        with tuned("s3_rt4", "s3_deep4", "s3_tile"):
            for rt, deep in ((8, 0), (8, 1), (7, 1), (6, 0), (5, 1), (4, 0), (3, 1), (2, 0), (2, 1), (0, 1)):
                tune("s3_rt4", rt)
                tune("s3_deep4", deep)
                tune("s3_tile", 1)
                outs[rt, deep] = (Fn.linear_bf16x3(x3, M, w3, N, K, bias=b.to(dev)).cpu(),
                                  Fn.linear_bf16x3(x3, M, w3, N, K, bias=b.to(dev), residual=r.to(dev)).cpu(),
                                  Fn.linear_bf16x3(x3, M, w3, N, K, bias=b.to(dev), act=L.ACT_GELU, out_split3=True).cpu())
        base = outs[8, 0]
        bound = 2.0 * K * 2.0 ** -24 * (x.double().abs() @ w.double().abs().t() + b.double().abs()) + 1e-30
        assert ((base[0].double() - ref).abs() <= bound).all(), (M, float(((base[0].double() - ref).abs() / bound).max()))
        assert ((base[1].double() - ref - r.double()).abs() <= bound + 2.0 ** -23 * (ref + r.double()).abs()).all(), M
        for key, o in outs.items():
            for which in range(3):
                assert torch.equal(o[which], base[which]), (M, key, which)


# ------------------------------------------------------------------------------------------------- bf16x3 adversarial suite
def _bf16x3_vs_f32(dev, x, w, b=None, strict=False):
    """(bf16x3 result, fp32-MFMA result, fp64 reference, sum_k |x_k w_k|) for y = x w^T (+ b)."""
    from multimodal_diffusion_amd import functional as Fn
    M, K = x.shape
    N = w.shape[0]
    y3 = Fn.linear_bf16x3(Fn.split3(x.to(dev)), M, Fn.split3(w.to(dev)), N, K, bias=None if b is None else b.to(dev),
                          terms=9 if strict else 6).cpu().double()
    y32 = Fn.linear(x.to(dev), w.to(dev), None if b is None else b.to(dev)).cpu().double()
    ref = x.double() @ w.double().t()
    if b is not None:
        ref = ref + b.double()
    mag = x.double().abs() @ w.double().abs().t()
    return y3, y32, ref, mag


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("scale", [1e-30, 1e-20, 1.0, 1e15, 3e18])
def test_bf16x3_dynamic_range(dev, scale, strict):
    """Operands from 1e-30 up to products near the top of the fp32 range: the split-operand GEMM stays within the fp32
    FMA chain's error bound (gamma_K * sum|x w|) and no worse than 2x the fp32-MFMA kernel's own error."""
    g = torch.Generator().manual_seed(int(abs(math.log10(scale))) + 3)
    M, N, K = 300, 256, 512
    x = torch.randn(M, K, generator=g) * scale
    w = torch.randn(N, K, generator=g) * (1.0 / math.sqrt(K)) * (scale if scale > 1 else 1.0)
    y3, y32, ref, mag = _bf16x3_vs_f32(dev, x, w, strict=strict)
    assert torch.isfinite(y3).all()
    bound = 2.0 * K * 2.0 ** -24 * mag            # a generous multiple of the fp32 dot-product bound
    assert ((y3 - ref).abs() <= bound).all()
    e3, e32 = (y3 - ref).abs().max().item(), (y32 - ref).abs().max().item()
    assert e3 <= 2.0 * e32 + 1e-30, (e3, e32)


@pytest.mark.parametrize("strict", [False, True])
def test_bf16x3_top_of_range_and_exact_bf16(dev, strict):
    """(a) values above the largest finite bf16 (3.3895e38 < |x| <= FLT_MAX) must not turn into infinities: their high plane is
    clamped and the remainder moves to the middle plane; (b) operands that ARE bf16 numbers (m = l = 0 planes) and small
    integers give exact results."""
    from multimodal_diffusion_amd import functional as Fn
    K, N = 64, 256
    x = torch.zeros(4, K)
    x[0, 0], x[0, 1] = 3.4e38, -3.39e38                 # both round to +-inf in bf16
    x[1, 0] = torch.finfo(torch.float32).max
    x[2, 8:40] = 3.0e38                                 # 32 huge terms whose weighted sum (1.5e38) still fits
    x[3, 5] = -torch.finfo(torch.float32).max
    w = torch.zeros(N, K)
    w[:, 0], w[:, 1], w[:, 5] = 0.5, 0.25, 1.0
    w[:, 8:40] = 1.0 / 64.0
    y3, y32, ref, _ = _bf16x3_vs_f32(dev, x, w, strict=strict)
    assert torch.isfinite(y3).all()
    assert rel_err(y3, ref) < 1e-6 and rel_err(y32, ref) < 1e-6
    # the image itself: planes still sum to x exactly
    pl = _split3_decode(Fn.split3(x.to(dev)).cpu().numpy(), 4, K).astype(np.float64)
    assert np.array_equal(pl.sum(0), x.numpy().astype(np.float64)) and np.isfinite(pl).all()
    # exact bf16 / integer operands: every product and partial sum is representable, so all three results are identical
    g = torch.Generator().manual_seed(4)
    xi = torch.randint(-8, 9, (130, 512), generator=g).float()
    wi = torch.randint(-4, 5, (256, 512), generator=g).float()
    y3, y32, ref, _ = _bf16x3_vs_f32(dev, xi, wi, strict=strict)
    assert torch.equal(y3, ref) and torch.equal(y32, ref)
    xb = torch.randn(130, 512, generator=g).bfloat16().float()
    wb = (torch.randn(256, 512, generator=g) / 16).bfloat16().float()
    y3, y32, ref, mag = _bf16x3_vs_f32(dev, xb, wb, strict=strict)
    assert ((y3 - ref).abs() <= 512 * 2.0 ** -24 * mag).all() and (y3 - ref).abs().max() <= 1.5 * (y32 - ref).abs().max() + 1e-12


@pytest.mark.parametrize("strict", [False, True])
def test_bf16x3_cancellation(dev, strict):
    """K-long catastrophic cancellation: products come in +a, -a pairs with a tiny residue, so the exact answer is ~1e-7 of
    sum|x w|.  Neither path can beat the fp32 dot-product bound here; bf16x3 must not be worse than the fp32-MFMA kernel by
    more than the terms it drops (6-term: 3 * 2^-24 per product; 9-term: none)."""
    g = torch.Generator().manual_seed(9)
    M, N, K = 260, 256, 2048
    a = torch.randn(M, K // 2, generator=g) * 100.0
    x = torch.empty(M, K)
    x[:, 0::2], x[:, 1::2] = a, -a
    x[:, 1::2] += torch.randn(M, K // 2, generator=g) * 1e-5          # tiny residue
    w = torch.empty(N, K)
    wv = torch.randn(N, K // 2, generator=g)
    w[:, 0::2], w[:, 1::2] = wv, wv
    y3, y32, ref, mag = _bf16x3_vs_f32(dev, x, w, strict=strict)
    e3, e32 = (y3 - ref).abs(), (y32 - ref).abs()
    assert (e32 <= K * 2.0 ** -24 * mag).all()
    assert (e3 <= (K + 8) * 2.0 ** -24 * mag).all()
    assert e3.max() <= 2.0 * e32.max(), (e3.max().item(), e32.max().item())


def test_bf16x3_tiny_values_document_the_floor(dev):
    """Below ~2^-110 the lower planes leave bf16's range (bf16 shares fp32's exponent range but has 7 mantissa bits), so the
    split is no longer exact: the ABSOLUTE error stays below 2^-126 per product — invisible unless every product of a dot
    product is that small.  This is the documented domain limit of the mode."""
    g = torch.Generator().manual_seed(12)
    x = torch.randn(64, 64, generator=g) * 1e-36
    w = torch.randn(256, 64, generator=g)
    y3, y32, ref, mag = _bf16x3_vs_f32(dev, x, w)
    assert torch.isfinite(y3).all()
    assert (y3 - ref).abs().max() <= 64 * 2.0 ** -126 * 8          # absolute floor, not relative accuracy
    assert (y32 - ref).abs().max() <= 64 * 2.0 ** -149 * 8 + 64 * 2.0 ** -24 * mag.max()


def test_bf16x3_nonfinite_rows_stay_local(dev):
    """inf / NaN in one input row make exactly that output row non-finite in both kernels (bf16x3 may report NaN where the
    fp32 chain reports +-inf: inf * 0-plane); every other row is untouched and still fp32-accurate."""
    g = torch.Generator().manual_seed(13)
    x = torch.randn(300, 256, generator=g)
    w = torch.randn(256, 256, generator=g) / 16
    x[5, 17] = float("inf")
    x[77, 3] = float("nan")
    x[200, 0] = float("-inf")
    y3, y32, ref, _ = _bf16x3_vs_f32(dev, x, w)
    bad = torch.tensor([5, 77, 200])
    good = torch.ones(300, dtype=torch.bool)
    good[bad] = False
    assert not torch.isfinite(y3[bad]).any() and not torch.isfinite(y32[bad]).any()
    assert torch.isfinite(y3[good]).all() and rel_err(y3[good], ref[good]) < 2e-6
    assert torch.isnan(y3[77]).all() and torch.isnan(y32[77]).all()


# ------------------------------------------------------------------------------------------------- drop-in corners (G16)
def test_dropin_corners_golden(dev, small_model):
    """key_padding_mask, norm="layernorm", relu / leaky_relu heads, variational eval encode and Hann overlap-add against the
    reference's own outputs (tests/golden/g16_dropin_corners.npz)."""
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import ops
    g, W, meta = small_model
    g16 = load_golden("g16_dropin_corners.npz")
    core, _, _, _ = _small_modules(dev, W, meta)
    y = core(G(g16["mask/x"], dev), key_padding_mask=G(g16["mask/kpm"], dev))
    assert rel_err(y.cpu(), g16["mask/y"]) < TOL
    assert rel_err(core.blocks[0](G(g16["mask/x"], dev), key_padding_mask=G(g16["mask/kpm"], dev)).cpu(),
                   R.mmdit_block(T(g16["mask/x"]), W["core"], "blocks.0.", meta["n_heads"], T(g16["mask/kpm"]))) < TOL
    ln = A.MMDiT(d_model=128, n_layers=2, n_heads=2, mlp_ratio=2.0, norm="layernorm").eval()
    ln.load_state_dict(grp(g16, "ln_core"), strict=True)
    assert rel_err(ln.to(dev)(G(g16["ln/x"], dev)).cpu(), g16["ln/y"]) < TOL
    for act in ("relu", "leaky_relu"):
        hd = A.MultiModalNoiseHead({"video": 128, "audio": 128}, {"video": 256, "audio": 32}, hidden_dim=64, activation=act).eval()
        hd.load_state_dict(grp(g16, f"head_{act}_w"), strict=True)
        out = hd.to(dev)({"video": G(g16[f"head_{act}/hv"], dev)})["video"]
        assert rel_err(out.cpu(), g16[f"head_{act}/out_v"]) < TOL
    vv = A.VideoVAE.from_config({"latent": {"channels": 8, "t_down": 4, "s_down": 8}, "variational": True}).eval()
    missing, unexpected = vv.load_state_dict(grp(g16, "vvae_w"), strict=False)
    assert not unexpected and all(k.startswith(("dec_net", "from_lat", "to_img")) for k in missing)
    vv = vv.to(dev)
    z = vv.encode(G(g16["vvae/x"], dev))
    assert z.shape == (2, 8, 2, 2, 3) and rel_err(z.cpu(), g16["vvae/z"]) < TOL
    assert abs(float(vv.kld_loss()) - float(g16["vvae/kld"])) < 1e-4
    y = ops.overlap_add_1d(G(g16["hann/windows"], dev), stride=4, apply_hann=True)
    assert rel_err(y.cpu(), g16["hann/y"]) < 1e-6
    assert rel_err(ops.overlap_add_1d(G(g16["hann/windows"], dev), stride=3).cpu(), g16["hann/y_rect"]) < 1e-6


def test_attention_key_padding_mask(dev):
    """Masked keys at tile boundaries, a fully kept and an almost fully masked sample, against masked softmax in fp64."""
    from multimodal_diffusion_amd import functional as Fn
    g = torch.Generator().manual_seed(23)
    B, N, H = 4, 200, 2
    d = 64 * H
    qkv = torch.randn(B, N, 3 * d, generator=g)
    kpm = torch.zeros(B, N, dtype=torch.bool)
    kpm[0, 64:128] = True            # one whole key tile
    kpm[1, 1:] = True                # a single visible key
    kpm[2, torch.randint(0, N, (90,), generator=g)] = True
    q, k, v = (qkv.double().view(B, N, 3, H, 64)[:, :, i].transpose(1, 2) for i in range(3))
    s = (q @ k.transpose(-1, -2) / 8.0).masked_fill(kpm[:, None, None, :], float("-inf"))
    ref = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, N, d)
    out = Fn.attention(qkv.to(dev), H, key_padding_mask=kpm.to(dev))
    assert rel_err(out.cpu(), ref) < 2e-5
    assert torch.equal(Fn.attention(qkv.to(dev), H, key_padding_mask=torch.zeros(B, N, dtype=torch.bool, device=dev)),
                       Fn.attention(qkv.to(dev), H))


@pytest.mark.parametrize("size,B", [(128, 32), (128, 7), (256, 9)])
def test_split_gemm_short_four_wave_blocks_agree(dev, full, size, B):
    """Round 4, VERDICT r3 next-round 4 (mid-size batches): the 4-wave bf16x3 blocks of in_proj / fc1 / out_proj / fc2 with 160, 192 or
    224 rows instead of 256 (avd_tune_set "s3_rt4" 5 / 6 / 7; 0 = the host picks per launch), and 64 / 96 / 128 rows for out_proj / fc2
    (2 / 3 / 4; in_proj and fc1 then take 5).  A block then starts at any multiple of
    32 rows, stages only its live A pieces and leaves row tiles dead — the MFMA sequence per output element is the one of the 256-row
    blocks, so a whole CFG step is bit-identical for every choice.  128 x 128 at B = 32: the reference's shipped geometry (8,512 rows:
    the automatic choice differs per launch — 5 for out_proj / fc2, 6 for fc1, 7 for in_proj); B = 7: 1,862 rows, ragged in every block
    size; 256 x 256 at B = 9: 7,578 rows."""
    from multimodal_diffusion_amd import _lib as L
    ws, mods = full
    core, head, av, aa = mods
    g = torch.Generator().manual_seed(177 + B)
    z_v = torch.randn(B, 8, 12, size // 8, size // 8, generator=g)
    z_a = torch.randn(B, 8, 150, generator=g)
    abar = R.alpha_bar_table(R.beta_table(1000))
    tn = torch.tensor(([982, 500, 16, 999] * B)[:B])
    tp = torch.tensor(([966, 480, -1, 979] * B)[:B])
    outs, names = {}, {}
    for rt, deep in ((8, 0), (8, 1), (7, 0), (6, 0), (5, 0), (5, 1), (6, 1), (4, 0), (4, 1), (3, 0), (3, 1), (2, 0), (2, 1), (0, 1)):
        with tuned(s3_rt4=rt, s3_deep4=deep, s3_min_rows=1, s3_tile=1):
            eng = engine((core, head, av, aa), "video", tuple(z_v.shape), 37, alpha_bar=abar, guidance=3.5, matmul="bf16x3")
            eng.set_prompt(z_a.to(dev))
            L.prof_enable(True)
            outs[rt, deep] = eng.step(z_v.to(dev), tn.to(dev), tp.to(dev)).cpu()
            torch.cuda.synchronize()
            L.prof_enable(False)
            names[rt, deep] = sorted(k[len("gemm_bf16x3_m16_kernel"):] for k, v in L.prof_report().items() if k.startswith("gemm_bf16x3_m16_kernel") and v[0] > 0)
    base = outs[8, 0]
    assert torch.isfinite(base).all()
    for key, out in outs.items():
        rt, deep = key
        if rt:
            assert any(n.startswith(f"<6, 4, {rt}, ") for n in names[key]), (key, names[key])       # (EPI 6 = residual + image: out_proj / fc2)
        if rt and deep:         # one block per CU on the four-stage ring wherever the launch's blocks fit the CUs once
            nv = 6 * (size // 32) ** 2                  # (the trimmed last block runs on the 2 B nv target rows, the others on 2 B (nv + 37))
            fits = [(2 * B * n + 32 * rt - 1) // (32 * rt) * 4 <= 256 for n in (nv, nv + 37)]
            assert (f"<6, 4, {rt}, 4>" in names[key]) == any(fits) and (f"<6, 4, {rt}, 0>" in names[key]) == (not all(fits)), (key, names[key])
        assert torch.equal(out, base), (key, float((out - base).abs().max()))
    print(f"short 4-wave blocks, {size}x{size} B={B}: automatic choice ran {names[0, 1]}")
    ref = R.denoise_step_a2v(z_v[:1], z_a[:1], tn[:1], tp[:1], abar, adapt_v=ws["adapt_v"], adapt_a=ws["adapt_a"], core=ws["core"],
                             head=ws["head"], n_layers=8, n_heads=8, guidance=3.5)
    assert rel_err(outs[5, 1][:1], ref) < TOL


@pytest.mark.parametrize("size,B", [(256, 32), (256, 5), (512, 8)])
def test_split_gemm_block_rows_agree(dev, full, size, B):
    """bf16x3 out_proj / fc2 (residual + image + row sums epilogue, 8 waves): the 224-row blocks the host picks when they fit one
    generation of blocks on the CUs (avd_tune_set "s3_rt" 0 / 7 / 8) read the operand images at row offsets that are multiples of
    32, not of 128, and leave the last row tile of each wave pair dead — same MFMA sequence per output element, so a whole CFG step is
    bit-identical with 256-row blocks.  B = 32: the bench shape (26,944 rows, last block past the last 128-row group);
    B = 5: 4,210 rows with the 8-wave blocks forced (18.8 blocks of 224 rows); 512x512, B = 8: the C5 geometry (25,168 rows, 1,573 tokens)."""
    ws, mods = full
    core, head, av, aa = mods
    g = torch.Generator().manual_seed(77 + B)
    z_v = torch.randn(B, 8, 12, size // 8, size // 8, generator=g)
    z_a = torch.randn(B, 8, 150, generator=g)
    abar = R.alpha_bar_table(R.beta_table(1000))
    tn = torch.tensor(([982, 500, 16, 999] * B)[:B])
    tp = torch.tensor(([966, 480, -1, 979] * B)[:B])
    outs = {}
    for rt, w128 in ((7, 0), (8, 0), (0, 0), (7, 1), (8, 1), (6, 1), (0, 1)):
        with tuned(s3_rt=rt, s3_w128=w128, s3_tile=0 if B == 5 else -1):
            eng = engine((core, head, av, aa), "video", tuple(z_v.shape), 37, alpha_bar=abar, guidance=3.5, matmul="bf16x3")
            eng.set_prompt(z_a.to(dev))
            outs[rt, w128] = eng.step(z_v.to(dev), tn.to(dev), tp.to(dev)).cpu()
    assert torch.isfinite(outs[7, 0]).all()
    assert torch.equal(outs[7, 0], outs[8, 0])
    assert torch.equal(outs[0, 0], outs[8, 0])
    # the 4-wave kernel with a 128 x 128 wave tile (avd_tune_set "s3_w128") issues the same MFMA sequence per output element
    assert torch.equal(outs[7, 1], outs[8, 0])
    assert torch.equal(outs[8, 1], outs[8, 0])
    # 192-row blocks (round 4: what the host picks for the trimmed last block, 24,576 rows) and the automatic choice
    assert torch.equal(outs[6, 1], outs[8, 0]) and torch.equal(outs[0, 1], outs[8, 0])
    outs = {7: outs[7, 0]}
    ref = R.denoise_step_a2v(z_v[:1], z_a[:1], tn[:1], tp[:1], abar, adapt_v=ws["adapt_v"], adapt_a=ws["adapt_a"], core=ws["core"],
                             head=ws["head"], n_layers=8, n_heads=8, guidance=3.5)
    assert rel_err(outs[7][:1], ref) < TOL


@pytest.mark.parametrize("B", [5, 32])
def test_f16x2_rownorm_epilogue_matches_norm_kernel(dev, full, B):
    """f16x2, d = 512: out_proj / fc2 run on 128 x 512 blocks that own whole rows and finish the NEXT RMSNorm (mmdt.py:39-42 after
    the residual add of :97-98) in their epilogue — fp32 stream + the normalised image, no rmsnorm_split3 launch between blocks.
    Same expression per element as the norm kernel; only the order in which a row's squares are summed differs, so the step agrees
    with the unfused pipeline (avd_tune_set "no_fold" 1) to fp32 rounding, and with the CPU oracle to the parity tolerance.
    B = 5: 4,210 rows (ragged last 128-row block); B = 32: the bench shape."""
    ws, mods = full
    core, head, av, aa = mods
    g = torch.Generator().manual_seed(900 + B)
    z_v = torch.randn(B, 8, 12, 32, 32, generator=g)
    z_a = torch.randn(B, 8, 150, generator=g)
    abar = R.alpha_bar_table(R.beta_table(1000))
    tn = torch.tensor(([982, 500, 16, 999] * B)[:B])
    tp = torch.tensor(([966, 480, -1, 979] * B)[:B])
    outs = []
    for no_fold in (0, 1):
        with tuned(no_fold=no_fold):
            eng = engine((core, head, av, aa), "video", tuple(z_v.shape), 37, alpha_bar=abar, guidance=3.5, matmul="f16x2")
            eng.set_prompt(z_a.to(dev))
            outs.append(eng.step(z_v.to(dev), tn.to(dev), tp.to(dev)).cpu())
    assert torch.isfinite(outs[0]).all()
    d = rel_err(outs[0], outs[1])
    print(f"f16x2 row-norm epilogue vs norm kernel, B={B}: {d:.3e}")
    # (B = 5 sits under the split kernels' row threshold: since round 4 its fold arm is the norm-FOLDED fp32 path — every mode carries the
    # folded fp32 weights — against separate norm kernels: 4.3e-6 for a whole step)
    assert d < (3e-6 if B == 32 else 1e-5)
    idx = [0, B - 1]
    ref = R.denoise_step_a2v(z_v[idx], z_a[idx], tn[idx], tp[idx], abar, adapt_v=ws["adapt_v"], adapt_a=ws["adapt_a"], core=ws["core"],
                             head=ws["head"], n_layers=8, n_heads=8, guidance=3.5)
    assert rel_err(outs[0][idx], ref) < TOL


@pytest.mark.parametrize("matmul", ["bf16x3_strict", "bf16"])
def test_splitk_small_batch_fc2(dev, full, matmul):
    """BASELINE C2 geometry (64x64, B = 32: 3,904 rows).  fc2's 256x128 blocks cover a quarter of the CUs, so its K = 2,048 is cut
    into four slices (blockIdx.y) whose fp32 partial sums a reduction kernel adds in slice order before bias and residual, writing the
    stream, its operand image and the rows' sums of squares as the fused epilogue would (avd_tune_set "s3_splitk"; no atomics:
    repeatable bit for bit).  Against the unsplit launch only the summation order differs; the strict nine-term mode (exact operands,
    forced onto the split kernels at this size) is held to the parity tolerance against the CPU oracle."""
    ws, mods = full
    outs = []
    with tuned("s3_splitk", s3_min_rows=0):
        for ns in (4, 0, 4):
            tune("s3_splitk", ns)
            out, ref = _one_step(dev, mods, ws, 64, 32, 2, matmul=matmul)
            outs.append(out)
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[2])
    d = rel_err(outs[0], outs[1])
    e = rel_err(outs[0][:2], ref)
    print(f"split-K fc2 vs one launch, {matmul}: {d:.3e}; vs CPU oracle {e:.3e}")
    assert not torch.equal(outs[0], outs[1])      # the split path really ran (the summation order shows)
    if matmul == "bf16x3_strict":
        assert d < 3e-6
        assert e < TOL
    else:
        # one-plane operands: a 1e-7 change of the stream flips 8-bit operand roundings downstream, so two summation orders differ by
        # about the mode's own error (measured 1.1e-2 between them, 7.1e-3 / 7.5e-3 against the oracle): reported-error bound only
        assert e < 3e-2 and d < 3e-2


def test_split_gemm_tile_configurations_agree(dev):
    """The two block configurations of the split-operand GEMM (8 waves 256x256 / 4 waves 256x128, avd_tune_set "s3_tile") sum
    every output element over k in the same order with the same product terms: bit-identical results, in every mode, for the
    fp32 and the image epilogues, on a ragged row count and on K = 16 .. 2048 (ring prologue / tail with fewer tiles than stages,
    odd and even step counts)."""
    from multimodal_diffusion_amd import functional as Fn, _lib as L
    g = torch.Generator().manual_seed(41)
    for M, N, K in ((2701, 512, 512), (768, 256, 16), (515, 256, 48), (300, 512, 2048), (1024, 768, 80), (256, 256, 112)):
        x = torch.randn(M, K, generator=g).to(dev)
        w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev)
        b = torch.randn(N, generator=g).to(dev)
        r = torch.randn(M, N, generator=g).to(dev)
        ref = (x.double() @ w.double().T + b.double() + r.double()).cpu()
        for mode in ("bf16x3", "bf16x3_strict", "bf16", "f16x2"):
            outs = []
            for tile in (0, 1):
                with tuned(s3_tile=tile):
                    if mode == "f16x2":
                        x2, sx = Fn.split_f16x2(x)
                        w2, sw = Fn.split_f16x2(w)
                        y = Fn.linear_f16x2(x2, M, w2, N, K, sx * sw, bias=b, residual=r)
                        img = Fn.linear_f16x2(x2, M, w2, N, K, sx * sw, bias=b, act=L.ACT_GELU, out_scale=64.0)
                    else:
                        terms = {"bf16x3": 6, "bf16x3_strict": 9, "bf16": 1}[mode]
                        x3, w3 = Fn.split3(x), Fn.split3(w)
                        y = Fn.linear_bf16x3(x3, M, w3, N, K, bias=b, residual=r, terms=terms)
                        img = Fn.linear_bf16x3(x3, M, w3, N, K, bias=b, act=L.ACT_GELU, out_split3=True, terms=terms)
                outs.append((y, img))
            assert torch.equal(outs[0][0], outs[1][0]), (mode, M, N, K)
            if M % 256 == 0:          # whole image defined (rows past M inside the last 256-row tile are never written)
                live = 2 if mode == "f16x2" else 3          # an f16x2 image never writes its third plane
                i0, i1 = (o[1].view(-1, 3, 4096)[:, :live] for o in outs)
                assert torch.equal(i0, i1), (mode, M, N, K)
            tol = 2e-2 if mode == "bf16" else 3e-6
            assert rel_err(outs[0][0].cpu(), ref) < tol, (mode, M, N, K)


# ------------------------------------------------------------------------------------------------- reduced-precision variants
@pytest.mark.parametrize("size,B,n_ref", [(64, 32, 2), (512, 8, 1)])
def test_bf16_mode_reported_error(dev, full, size, B, n_ref):
    """BASELINE configs C2 (64x64, B=32) and C5 geometry (512x512, B=8) with matmul="bf16": plain bf16 operands, fp32
    accumulation, in the block projections and the attention.  NOT a parity path — the reference has no reduced-precision
    inference (sample_clip.py:399-411 never reads mixed_precision).  The test states the error against the fp32 oracle: one
    CFG step stays within 3e-2 of the oracle relative to max|z|, and is measurably different from the fp32 path (so the
    mode really ran)."""
    ws, mods = full
    out, ref = _one_step(dev, mods, ws, size, B, n_ref, matmul="bf16")
    err = rel_err(out[:n_ref], ref)
    print(f"bf16 mode {size}x{size} B={B}: rel err vs fp32 oracle {err:.3e}")
    assert 1e-5 < err < 3e-2


@pytest.mark.parametrize("B,N,H", [(1, 64, 4), (2, 133, 4), (1, 421, 8), (1, 1573, 4)])
def test_attention_fp8_reported_error(dev, B, N, H):
    """fp8 (e4m3) attention against softmax(q k^T / 8) v in fp64: the kernel is correct when its error is that of rounding
    q, k, v and p to 4 significant bits — measured 8-10 % of max|out| on N(0, 1.5^2) operands, whose scores are far peakier than the
    model's — and nowhere near the O(1) error a wrong operand map gives.  Second figure: against an fp64 evaluation on the SAME
    e4m3-rounded q, k, v and a p rounded to e4m3 (isolates the kernel from the operand quantisation; the residue is the online
    softmax rounding p against running maxima): 0.6-2 %."""
    from multimodal_diffusion_amd import functional as Fn, _lib as L
    d = H * 64
    g = torch.Generator().manual_seed(B * 100 + N + H)
    qkv = torch.randn(B * N, 3 * d, generator=g) * 1.5
    lib = L.lib()
    img = torch.empty(lib.avd_qkv3_bytes(B, N, H), dtype=torch.uint8, device=dev)
    x3, w3 = Fn.split3(qkv.to(dev)), Fn.split3(torch.eye(3 * d).to(dev))
    zb = torch.zeros(3 * d, device=dev)
    qs = 0.125 * 1.4426950408889634
    L.check(lib.avd_gemm_bf16x3_qkv3_f32(x3.data_ptr(), w3.data_ptr(), zb.data_ptr(), img.data_ptr(), B * N, N, H, 3 * d, qs, 6,
                                         L.stream_ptr(dev)))
    ws = torch.empty(lib.avd_attn_fp8_workspace_bytes(B, N, H), dtype=torch.uint8, device=dev)
    out = torch.full((B, N, d), 7.0, device=dev)
    nq = N if N < 400 else N - 37
    L.check(lib.avd_attn_fwd_fp8_f32(img.data_ptr(), ws.data_ptr(), ws.numel(), out.data_ptr(), None, B, N, H, nq, L.stream_ptr(dev)))
    full = qkv.double().view(B, N, 3, H, 64)
    q, k, v = (full[:, :, i].transpose(1, 2) for i in range(3))
    ref = (torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1) @ v).transpose(1, 2).reshape(B, N, d)
    err = rel_err(out.cpu()[:, :nq], ref[:, :nq])
    # fp64 on the operands the kernel actually multiplies (q carries scale * log2 e * 8 before its rounding)
    f8 = lambda t: t.float().to(torch.float8_e4m3fn).double()
    qq = f8(q * (qs * 8.0))
    s = (qq @ f8(k).transpose(-1, -2)) / 8.0 * math.log(2.0)
    p = torch.softmax(s, dim=-1)
    pq = f8(p / p.max(-1, keepdim=True).values * 256.0) / 256.0 * p.max(-1, keepdim=True).values      # p is rounded relative to the row max
    ref8 = (pq @ f8(v) / p.sum(-1, keepdim=True)).transpose(1, 2).reshape(B, N, d)
    err8 = rel_err(out.cpu()[:, :nq], ref8[:, :nq])
    print(f"fp8 attention B={B} N={N} H={H}: rel err vs fp64 {err:.3e}, vs fp64 on the e4m3 operands {err8:.3e}")
    # measured (round 4, GPU box): err 8.2e-2 / 7.7e-2 / 9.5e-2 / 8.9e-2 (operand quantisation on N(0, 1.5^2) data), err8 6.3e-3 / 1.1e-2 /
    # 2.1e-2 / 1.6e-2 for N = 64 / 133 / 421 / 1573; the bounds sit at 1.3x resp. 2x of that — a wrong operand map inside a lane group is O(1)
    bound, bound8 = {64: (0.11, 1.3e-2), 133: (0.10, 2.3e-2), 421: (0.125, 4.2e-2), 1573: (0.12, 3.3e-2)}[N]
    assert err < bound and err8 < bound8
    assert torch.all(out[:, nq:] == 7.0)


def test_fp8_attention_step_c5(dev, full):
    """BASELINE C5 geometry (512x512: 1536 + 37 tokens), B=8 per GPU, bf16x3 projections + fp8 attention: one CFG step against the
    fp32 oracle on sample 0 — reported error, bound 3e-3 of max|z| = 2.2x the measured 1.35e-3 (the fp32 paths sit at 2e-6)."""
    ws, mods = full
    import multimodal_diffusion_amd as A
    core, head, av, aa = mods
    g = torch.Generator().manual_seed(512)
    B = 8
    z_v = torch.randn(B, 8, 12, 64, 64, generator=g)
    z_a = torch.randn(B, 8, 150, generator=g)
    abar = R.alpha_bar_table(R.beta_table(1000))
    tn = torch.tensor([982, 500, 16, 999] * 2)
    tp = torch.tensor([966, 480, -1, 979] * 2)
    ref = R.denoise_step_a2v(z_v[:1], z_a[:1], tn[:1], tp[:1], abar, adapt_v=ws["adapt_v"], adapt_a=ws["adapt_a"], core=ws["core"],
                             head=ws["head"], n_layers=8, n_heads=8, guidance=3.5)
    outs = {}
    for attn in ("default", "fp8"):
        eng = engine((core, head, av, aa), "video", tuple(z_v.shape), 37, alpha_bar=abar, guidance=3.5, matmul="bf16x3", attn=attn)
        eng.set_prompt(z_a.to(dev))
        outs[attn] = eng.step(z_v.to(dev), tn.to(dev), tp.to(dev)).cpu()
    e_def, e_f8 = rel_err(outs["default"][:1], ref), rel_err(outs["fp8"][:1], ref)
    print(f"C5 step: bf16x3 attention rel err {e_def:.3e}, fp8 attention rel err {e_f8:.3e}")
    assert e_def < TOL and 1e-5 < e_f8 < 3e-3            # measured 1.35e-3 (round 4); the fp32-level paths sit at 2e-6
    with pytest.raises(ValueError):
        engine((core, head, av, aa), "video", tuple(z_v.shape), 37, alpha_bar=abar, guidance=3.5, matmul="f32", attn="fp8")
    # an fp8 request on a core the split-operand kernels do not take (d = 384: 3d % 256 != 0) is refused, not run in fp32
    from multimodal_diffusion_amd import _lib as L
    narrow = A.MMDiT(d_model=384, n_layers=1, n_heads=6).to(dev).eval()
    narrow.matmul, narrow.attn = "bf16x3", "fp8"
    with pytest.raises(L.AvdError, match="fp8 attention"):
        narrow(torch.randn(2, 64, 384, device=dev))
    narrow.attn = "default"
    assert torch.isfinite(narrow(torch.randn(2, 64, 384, device=dev))).all()     # same core without the request: fp32 kernels
