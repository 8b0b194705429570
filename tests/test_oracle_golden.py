"""CPU: pins the oracle (oracle/ref_cpu.py) to golden vectors produced by the reference itself
(tools/make_golden.py) and to the reference's own value-level test (patch/unpatch round trip,
reference tests/test_shapes.py:26-36)."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

from _kit import grp
from conftest import load_golden, rel_err, split_weights
from oracle import ref_cpu as R

TOL = 1e-4   # max|Δ| <= TOL * max(1, max|ref|)   


def _mkl_branch():
    """The code branch (MKL_CBWR_* value) MKL's vector math runs in this process, or None: torch's CPU exp / sin / cos go through it."""
    try:
        lib = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libtorch_cpu.so"))
        forced = int(lib.mkl_serv_cbwr_get(1))              # MKL_CBWR_BRANCH: a branch MKL_CBWR forced, else 1 / 2 (off / auto)
        return forced if forced > 2 else int(lib.mkl_serv_cbwr_get_auto_branch())
    except (OSError, AttributeError):
        return None


# The reference's fp32 timestep embedding was recorded on MKL's AVX-512 branch for Intel CPUs (MKL_CBWR_AVX512 = 12, _AVX512_E1 = 14):
# there the oracle reproduces it bit for bit.  Other branches round a few exp / sin / cos results differently, and t up to 999
# magnifies a one-ulp change of a frequency a thousandfold in the angle; temb_ulp_bound is what that allows.
GOLDEN_BRANCH = _mkl_branch() in (12, 14)


def temb_ulp_bound(t, dim):
    """Largest change of R.timestep_embedding(t, dim) when each frequency moves by one ulp, each angle t * f rounds the other way and
    each cos / sin is one ulp off on both sides: |t| ulp(f) + ulp(t f) + 2 ulp(1), per element (the odd-dim pad column is exact)."""
    half = dim // 2
    t = np.abs(np.asarray(t, dtype=np.float64))[:, None]
    f = np.exp(-math.log(10000) * np.arange(half) / half).astype(np.float32)[None]
    b = t * np.spacing(f) + np.spacing((t * f).astype(np.float32)) + 2 * np.spacing(np.float32(1))
    return np.pad(np.concatenate([b, b], 1), ((0, 0), (0, dim % 2)))


def T(a):
    return torch.from_numpy(np.asarray(a))


def test_g1_schedules_bit_exact():
    g = load_golden("g1_schedules.npz")
    for kind in ("cosine", "linear", "sigmoid"):
        b = R.beta_table(1000, kind, 1e-4, 0.02)
        assert np.array_equal(b.numpy(), g[f"betas/{kind}"]), kind
        assert np.array_equal(R.alpha_bar_table(b).numpy(), g[f"abar/{kind}"]), kind
    for S in (10, 25, 50, 60, 100):
        assert np.array_equal(R.sampling_schedule(1000, S).numpy(), g[f"sched/{S}"])
    assert np.array_equal(R.sampling_schedule(50, 7).numpy(), g["sched/T50_S7"])
    ab = g["abar/cosine"]
    # spot values quoted in SURVEY §8c
    assert abs(ab[0] - 0.99995875) < 1e-7 and abs(ab[500] - 0.49228531) < 1e-7
    assert g["sched/60"][0] == 999 and g["sched/60"][1] == 982 and g["sched/60"][-1] == -1


def test_g2_timestep_embedding():
    g = load_golden("g2_temb.npz")
    t = T(g["t"])
    for dim, key in ((256, "e256"), (64, "e64"), (7, "e7")):
        got = R.timestep_embedding(t, dim).numpy()
        assert (np.abs(got - g[key]) <= temb_ulp_bound(g["t"], dim)).all(), dim
        if GOLDEN_BRANCH:
            assert np.array_equal(got, g[key]), dim
    e0 = R.timestep_embedding(torch.zeros(1, dtype=torch.long), 256)[0]
    assert torch.equal(e0[:128], torch.ones(128)) and torch.equal(e0[128:], torch.zeros(128))


def test_g3_index_maps_exact():
    g = load_golden("g3_index.npz")
    for key in [k for k in g if k.startswith("patch/")]:
        C, Tt, H, W = map(int, key.split("/")[1].split("x"))
        z = torch.arange(C * Tt * H * W, dtype=torch.float32).view(1, C, Tt, H, W)
        tok = R.tube_patch(z, 2, 4, 4)
        assert np.array_equal(tok.numpy().astype(np.int32), g[key])
        assert torch.equal(R.tube_unpatch(tok, C, Tt, H, W, 2, 4, 4), z)
    za = torch.arange(2 * 8 * 150, dtype=torch.float32).view(2, 8, 150)
    tok = R.audio_tokens(za, 4, 4)
    assert np.array_equal(tok.numpy().astype(np.int32), g["audio_tok/150"])
    un = R.audio_untokens(tok + 1.0, 8, 4, 150, 4)
    assert np.array_equal(un.numpy().astype(np.int32), g["audio_untok/150"])
    assert torch.equal(un[..., 148:], torch.zeros(2, 8, 2))       # zero tail (sample_clip.py:213-214)
    zb = T(g["audio22/z"])
    assert np.array_equal(R.audio_tokens(zb, 4, 4).numpy(), g["audio22/tok"])
    assert np.array_equal(R.audio_untokens(T(g["audio22/tok"]), 8, 4, 22, 4).numpy(), g["audio22/untok"])
    assert np.array_equal(R.audio_tokens(zb, 4, 2).numpy(), g["audio22s2/tok"])
    assert np.allclose(R.audio_untokens(T(g["audio22s2/tok"]), 8, 4, 22, 2).numpy(), g["audio22s2/untok"], atol=1e-6)


def test_reference_roundtrip_case():
    # same shapes/atol as the reference's tests/test_shapes.py:26-36
    torch.manual_seed(0)
    z = torch.randn(2, 8, 12, 16, 16)
    tok = R.tube_patch(z, 2, 4, 4)
    assert tok.shape == (2, 6 * 4 * 4, 256)
    assert torch.allclose(z, R.tube_unpatch(tok, 8, 12, 16, 16, 2, 4, 4), atol=1e-6)
    with pytest.raises(AssertionError):
        R.tube_patch(torch.zeros(1, 8, 3, 16, 16), 2, 4, 4)


def test_g4_rmsnorm():
    g = load_golden("g4_rmsnorm.npz")
    y = R.rmsnorm(T(g["x"]), T(g["scale"]))
    assert rel_err(y, g["y"]) < 1e-6
    assert torch.equal(y[2], torch.zeros(512))


def test_g5_block_and_core(small_model):
    g, W, meta = small_model
    core = W["core"]
    x = T(g["x"])
    assert rel_err(R.mmdit_block(x, core, "blocks.0.", meta["n_heads"]), g["y_block0"]) < TOL
    assert rel_err(R.mmdit_forward(x, core, meta["n_layers"], meta["n_heads"]), g["y"]) < TOL
    assert rel_err(R.mmdit_forward(T(g["x_b"]), core, meta["n_layers"], meta["n_heads"]), g["y_b"]) < TOL


def test_g6_head(small_model):
    _, W, _ = small_model
    g = load_golden("g6_head_small.npz")
    assert rel_err(R.noise_head(T(g["hv"]), W["head"], "video"), g["out_v"]) < TOL
    assert rel_err(R.noise_head(T(g["ha"]), W["head"], "audio"), g["out_a"]) < TOL


def test_g7_ddim():
    g = load_golden("g7_ddim.npz")
    y = R.ddim_update(T(g["x_t"]), T(g["t_now"]), T(g["t_prev"]), T(g["eps"]), T(g["abar"]))
    assert rel_err(y, g["x_prev"]) < 1e-6
    # t_prev = -1 -> alpha_bar_prev = 1 -> result is x0_pred exactly
    assert torch.isfinite(y).all()


@pytest.mark.parametrize("guide", [0.0, 1.0, 3.5])
def test_g8_cfg_step(small_model, guide):
    _, W, meta = small_model
    g = load_golden("g8_cfg_step_small.npz")
    kw = dict(adapt_v=W["adapt_v"], adapt_a=W["adapt_a"], core=W["core"], head=W["head"],
              n_layers=meta["n_layers"], n_heads=meta["n_heads"], tdim=meta["tdim"], guidance=guide)
    z_v, z_a, tn, tp, ab = (T(g[k]) for k in ("z_v", "z_a", "t_now", "t_prev", "abar"))
    zn, et = R.denoise_step_a2v(z_v, z_a, tn, tp, ab, return_eps=True, **kw)
    assert rel_err(et, g[f"a2v/g{guide}/eps_tok"]) < TOL
    assert rel_err(zn, g[f"a2v/g{guide}/z_next"]) < TOL
    zn, et = R.denoise_step_v2a(z_a, z_v, tn, tp, ab, return_eps=True, **kw)
    assert rel_err(et, g[f"v2a/g{guide}/eps_tok"]) < TOL
    assert rel_err(zn, g[f"v2a/g{guide}/z_next"]) < TOL


def test_g9_chained_sampler(small_model):
    _, W, meta = small_model
    g = load_golden("g9_chain_small.npz")
    z = R.sample_a2v(T(g["z_init"]), T(g["z_a0"]), T(g["sched"]), T(g["abar"]),
                     adapt_v=W["adapt_v"], adapt_a=W["adapt_a"], core=W["core"], head=W["head"],
                     n_layers=meta["n_layers"], n_heads=meta["n_heads"], tdim=meta["tdim"],
                     guidance=float(g["guidance"]))
    ref = T(g["z_final"]).double()
    rel_l2 = float((z.double() - ref).norm() / ref.norm())
    assert rel_l2 < 1e-3, rel_l2       # chained tolerance (first step gain x20,290)


def test_g10_timestep_mlp():
    g = load_golden("g10_tmlp.npz")
    W = split_weights(g)["w"]
    assert rel_err(R.timestep_mlp(T(g["t"]), W, 64), g["y"]) < 1e-5


def test_fp64_oracle_agrees_with_fp32(small_model):
    g, W, meta = small_model
    W64 = R.cast_weights(W, torch.float64)
    y64 = R.mmdit_forward(T(g["x"]).double(), W64["core"], meta["n_layers"], meta["n_heads"])
    assert rel_err(y64, g["y"]) < 1e-5


def test_g11_vae_decode():
    """Loop boundary (next-1): the oracle's VideoVAE.decode restatement vs the reference module's output."""
    g = load_golden("g11_vae_decode.npz")
    W = split_weights(g)["w"]
    assert rel_err(R.vae_decode(T(g["z"]), W), g["x"]) < 1e-5
    assert rel_err(R.vae_decode(T(g["z"][:1]), W, out_size=(6, 24, 40)), g["x_odd"]) < 1e-5
    # hand-written trilinear == torch's F.interpolate rule on an awkward size
    x = torch.randn(1, 2, 3, 5, 4, generator=torch.Generator().manual_seed(0))
    ref = torch.nn.functional.interpolate(x, size=(7, 9, 10), mode="trilinear", align_corners=False)
    assert rel_err(R.trilinear_upsample(x, (7, 9, 10)), ref) < 1e-6


def test_g12_vae_encode():
    g = load_golden("g12_vae_encode.npz")
    W = split_weights(g)["w"]
    assert rel_err(R.vae_encode(T(g["x"]), W), g["z"]) < 1e-5
    assert rel_err(R.vae_encode(T(g["x_crop"])[:, :, 0:8, 1:17, 0:16], W), g["z_crop"]) < 1e-5


def test_g13_audio_codec():
    g = load_golden("g13_audio_codec.npz")
    W = split_weights(g)["w"]
    assert rel_err(R.codec_encode(T(g["wav"]), W), g["z"]) < 1e-5
    assert rel_err(R.codec_decode(T(g["z_in"]), W), g["wav_out"]) < 1e-5


def test_g14_stream_stitch_oracle_and_host_split():
    """next-3: the cross-fade oracle and the product's host-side window splitting vs the reference's helpers."""
    from multimodal_diffusion_amd import stream_infer as S
    g = load_golden("g14_stream_stitch.npz")
    assert np.array_equal(R.crossfade(g["a_chunks"], S.audio_fade_window(1000, 250), 400), g["a_fade"])
    assert np.array_equal(R.crossfade(g["a_chunks"], S.audio_fade_window(1000, 0), 400), g["a_rect"])
    v = R.crossfade(g["v_chunks"].astype(np.float32) / 255.0, S.video_fade_window(12, 3), 4)
    assert np.array_equal((np.clip(v, 0, 1) * 255.0).astype(np.uint8), g["v_fade"])
    sa, wa, ha = S.split_audio_into_windows(g["y_long"], sr=1000, win_s=3.0, hop_s=1.0)
    sf, wf, hf = S.split_frames_into_windows(g["f_long"], fps=4, win_s=3.0, hop_s=1.0)
    assert np.array_equal(sa, g["split_a"]) and np.array_equal(sf, g["split_f"])
    assert [wa, ha, wf, hf] == list(g["split_meta"])
    one, _, _ = S.split_audio_into_windows(g["y_long"][:100], sr=1000, win_s=3.0, hop_s=1.0)
    assert one.shape == (1, 100)


def test_g15_add_mode_step(small_model):
    """next-4: the trainer's embedding (d-wide adapters + ADDED timestep embedding, train/trainer.py:36-49), one CFG step
    produced by the reference's own helper definitions (tools/make_golden.py G15)."""
    _, W, meta = small_model
    g = load_golden("g15_add_mode_step.npz")
    Wa = split_weights(g)
    z, eps = R.denoise_step_a2v(T(g["z_v"]), T(g["z_a"]), T(g["t_now"]), T(g["t_prev"]), T(g["abar"]), adapt_v=Wa["adapt_v"],
                                adapt_a=Wa["adapt_a"], core=W["core"], head=W["head"], n_layers=meta["n_layers"],
                                n_heads=meta["n_heads"], tdim=meta["tdim"], guidance=float(g["guidance"]), return_eps=True,
                                temb_mode="add")
    assert rel_err(eps, g["eps_tok"]) < TOL
    assert rel_err(z, g["z_next"]) < TOL
    tok_v = R.tube_patch(T(g["z_v"]), 2, 4, 4)
    Xv = R.embed_with_time(tok_v, Wa["adapt_v"]["proj.weight"], Wa["adapt_v"]["proj.bias"], T(g["t_now"]), 0, "add")
    X = g["X"][:, :tok_v.shape[1]]
    bound = temb_ulp_bound(g["t_now"], X.shape[-1])[:, None, :] + 1e-6 * max(1.0, float(np.abs(X).max()))
    assert (np.abs(Xv.numpy() - X) <= bound).all()
    if GOLDEN_BRANCH:
        assert rel_err(Xv, X) < 1e-6


def g17_inputs():
    """The seeded inputs of fixture g17 (tools/make_golden.py G17): weights = synth_weights(0), latents from seed 1717."""
    gen = torch.Generator().manual_seed(1717)
    z_v = torch.randn(8, 8, 12, 32, 32, generator=gen)
    z_a = torch.randn(8, 8, 150, generator=gen)
    return z_v, z_a


def test_g17_full_width_step():
    """One CFG step at the bench's full model width (d=512, L=8, H=8, 384+37 tokens) computed by the REFERENCE's own modules
    (weights by the seeded recipe, not stored): the oracle on the first two samples, eps tokens and next latents."""
    g = load_golden("g17_full_step_c3.npz")
    ws = R.synth_weights(seed=0)
    z_v, z_a = g17_inputs()
    abar = R.alpha_bar_table(R.beta_table(1000))
    z, eps = R.denoise_step_a2v(z_v[:2], z_a[:2], T(g["t_now"])[:2], T(g["t_prev"])[:2], abar, adapt_v=ws["adapt_v"], adapt_a=ws["adapt_a"],
                                core=ws["core"], head=ws["head"], n_layers=8, n_heads=8, guidance=3.5, return_eps=True)
    assert rel_err(eps[:1], g["eps_tok0"]) < TOL
    assert rel_err(z, g["z_next01"]) < TOL


def g18_inputs():
    """The seeded inputs of fixture g18 (tools/make_golden.py G18): core input, head video rows, head audio rows (seed 1818)."""
    gen = torch.Generator().manual_seed(1818)
    return (torch.randn(16, 421, 1024, generator=gen), torch.randn(64, 96, 1024, generator=gen), torch.randn(64, 37, 1024, generator=gen))


def test_g18_class_default_width():
    """The reference's class-default width (mmdt.py:125-126: d_model 1024, 16 heads; two layers) and its shape test's head
    (tests/test_shapes.py:86-107: d = 1024, Nv = 96, Na = 37) computed by the REFERENCE's own modules on seeded-recipe weights:
    the oracle on the first and last sample."""
    g = load_golden("g18_class_default_width.npz")
    meta = json.loads(str(g["meta"]))
    ws = R.synth_weights(seed=meta["seed_weights"], d=1024, n_layers=2)
    x, hv, ha = g18_inputs()
    y = R.mmdit_forward(x[[0, -1]], ws["core"], 2, 16)
    assert rel_err(y[0, ::8], g["core_first"]) < TOL and rel_err(y[1, ::8], g["core_last"]) < TOL
    ov = R.noise_head(hv[[0, -1]], ws["head"], "video")
    assert rel_err(ov[0], g["head_video_first"]) < TOL and rel_err(ov[1], g["head_video_last"]) < TOL
    assert rel_err(R.noise_head(ha[:1], ws["head"], "audio")[0], g["head_audio_first"]) < TOL


def g19_setup():
    """Fixture g19 (tools/make_golden.py G19): the reference's shipped config (mvp.yaml + a2v.yaml) through ITS OWN
    sample_one_direction(prompt_modality="audio").  Weights and the prompt are seeded recipes (not stored): returns
    (fixture, meta, core/head/adapter weights, VideoVAE weights, AudioCodec weights, prompt waveform)."""
    g = load_golden("g19_shipped_config_a2v.npz")
    meta = json.loads(str(g["meta"]))
    ws = R.synth_weights(seed=meta["seed_weights"])
    Wv = R.synth_like({k: tuple(v) for k, v in meta["vae_shapes"].items()}, meta["seed_vae"])
    Wc = R.synth_like({k: tuple(v) for k, v in meta["codec_shapes"].items()}, meta["seed_codec"])
    wav = (0.1 * torch.randn(48000, generator=torch.Generator().manual_seed(meta["seed_wav"]))).numpy().astype(np.float32)
    return g, meta, ws, Wv, Wc, wav


def frames_close(got_u8, ref_u8):
    """<= 1 LSB everywhere and different on < 0.1 % of the pixels"""
    diff = np.abs(got_u8.astype(np.int32) - ref_u8.astype(np.int32))
    return int(diff.max()), float((diff > 0).mean())


def test_g19_shipped_config_through_reference_sampler():
    """The oracle PIPELINE (codec encode -> 60 chained CFG + DDIM steps at d = 512, L = 8, 96 + 37 tokens -> VideoVAE decode -> uint8)
    against what the reference's own sample_one_direction produced on its unmodified shipped configuration (VERDICT r4 missing 4)."""
    g, meta, ws, Wv, Wc, wav = g19_setup()
    cfg = meta["cfg"]
    assert cfg["model"]["core"]["d_model"] == 512 and cfg["video"]["size"] == [128, 128] and cfg["diffusion"]["video"]["sampler_steps"] == 60
    z_a0 = R.codec_encode(torch.from_numpy(wav).view(1, 1, -1), Wc, frames_per_clip=cfg["audio"]["latent"]["frames_per_clip"],
                          hop=cfg["audio"]["codec"]["hop_samples"])
    assert rel_err(z_a0, g["z_a0"]) < TOL
    c = cfg["diffusion"]["video"]
    abar = R.alpha_bar_table(R.beta_table(c["steps"], c["schedule"], c["min_beta"], c["max_beta"]))
    z = R.sample_a2v(T(g["z_init"]), z_a0, R.sampling_schedule(c["steps"], c["sampler_steps"]), abar, adapt_v=ws["adapt_v"],
                     adapt_a=ws["adapt_a"], core=ws["core"], head=ws["head"], n_layers=8, n_heads=8,
                     guidance=cfg["sampling"]["guidance_scale"]["video"])
    ref = T(g["z_final"]).double()
    rel_l2 = float((z.double() - ref).norm() / ref.norm())
    assert rel_l2 < 1e-3, rel_l2       # chained tolerance; measured ~1e-6
    # decode every 6th frame's neighbourhood is not separable (3x3x3 convolutions, GroupNorm over the clip): decode all, compare the stored ones
    x = R.vae_decode(z, Wv).clamp(0, 1)
    frames = (x[0].permute(1, 2, 3, 0).numpy() * 255.0).astype(np.uint8)
    assert frames.shape == (48, 128, 128, 3)
    mx, frac = frames_close(frames[::meta["frame_stride"]], g["frames"])
    assert mx <= 1 and frac < 1e-3, (mx, frac)


def test_g16_dropin_corners(small_model):
    """Options of the reference API the shipped sampler never uses: key_padding_mask, norm="layernorm", relu / leaky_relu heads,
    variational eval encode, Hann-window overlap-add (tools/make_golden.py G16)."""
    _, W, meta = small_model
    g = load_golden("g16_dropin_corners.npz")
    y = R.mmdit_forward(T(g["mask/x"]), W["core"], meta["n_layers"], meta["n_heads"], key_padding_mask=T(g["mask/kpm"]))
    assert rel_err(y, g["mask/y"]) < TOL
    assert rel_err(R.mmdit_forward(T(g["ln/x"]), grp(g, "ln_core"), 2, 2), g["ln/y"]) < TOL
    for act in ("relu", "leaky_relu"):
        out = R.noise_head(T(g[f"head_{act}/hv"]), grp(g, f"head_{act}_w"), "video", activation=act)
        assert rel_err(out, g[f"head_{act}/out_v"]) < TOL
    z, kld = R.vae_encode(T(g["vvae/x"]), grp(g, "vvae_w"), variational=True)
    assert rel_err(z, g["vvae/z"]) < TOL and abs(float(kld) - float(g["vvae/kld"])) < 1e-5
    wnd = T(g["hann/windows"])                                         # [2,3,5,8] -> one "channel" per prefix row
    flat = wnd.reshape(6, 5, 8)
    y = R.audio_untokens(flat, 1, 8, 24, 4, hann=True).view(2, 3, 24)
    assert rel_err(y, g["hann/y"]) < 1e-6


def test_fast_port_matches_oracle(small_model):
    """bench.py's timed cpu_baseline (oracle/ref_cpu_fast.py: the same functions on the fused ATen kernels the reference's modules
    dispatch to) against the pinned oracle: every function to 1e-5, and the full-width CFG step against the REFERENCE's own output
    (fixture g17).  tools/cpu_port_speed.py holds its speed to the reference's (profiles/r03_cpu_port_speed.json)."""
    from oracle import ref_cpu_fast as RF
    g, W, meta = small_model
    L_, H_ = meta["n_layers"], meta["n_heads"]
    x = T(g["x"])
    assert rel_err(RF.mmdit_forward(x, W["core"], L_, H_), R.mmdit_forward(x, W["core"], L_, H_)) < 1e-5
    ws = R.synth_weights(seed=0, n_layers=2)
    gen = torch.Generator().manual_seed(5)
    xx = torch.randn(3, 61, 512, generator=gen)
    assert rel_err(RF.mmdit_forward(xx, ws["core"], 2, 8), R.mmdit_forward(xx, ws["core"], 2, 8)) < 1e-5
    assert rel_err(RF.rmsnorm(xx, ws["core"]["final_norm.scale"]), R.rmsnorm(xx, ws["core"]["final_norm.scale"])) < 1e-6
    assert rel_err(RF.noise_head(xx, ws["head"], "video"), R.noise_head(xx, ws["head"], "video")) < 1e-5
    # one full-width CFG step on g17's first two samples: port vs oracle and vs the reference's stored result
    g17 = load_golden("g17_full_step_c3.npz")
    wf = R.synth_weights(seed=0)
    z_v, z_a = g17_inputs()
    abar = R.alpha_bar_table(R.beta_table(1000))
    kw = dict(adapt_v=wf["adapt_v"], adapt_a=wf["adapt_a"], core=wf["core"], head=wf["head"], n_layers=8, n_heads=8, guidance=3.5)
    zf = RF.denoise_step_a2v(z_v[:2], z_a[:2], T(g17["t_now"])[:2], T(g17["t_prev"])[:2], abar, **kw)
    zo = R.denoise_step_a2v(z_v[:2], z_a[:2], T(g17["t_now"])[:2], T(g17["t_prev"])[:2], abar, **kw)
    assert rel_err(zf, zo) < 1e-5
    assert rel_err(zf, g17["z_next01"]) < TOL
