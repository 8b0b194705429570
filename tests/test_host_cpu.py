"""CPU-only checks (no GPU, no kernel launches): the C ABI library loads and exports every symbol the header
declares, host-side schedule tables are bit-identical to the reference's, module state_dict keys match the
reference's, the product refuses CPU tensors instead of falling back, and the sharding helpers are right."""
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from _tune import DEFAULTS
from conftest import ROOT, load_golden


def test_documented_tune_keys_are_accepted():
    """Every avd_tune_set key the header documents is one the library accepts (and an unknown key is refused): the keys are how
    DESIGN.md's measurements are reproduced, so a renamed or dropped knob must show up here.  Host-side state only: no GPU call."""
    from multimodal_diffusion_amd import _lib as L
    header = (ROOT / "include" / "avdiff_hip.h").read_text()
    block = header[header.index("Measurement / test hooks"):header.index("int         avd_tune_set")]
    keys = sorted(set(re.findall(r'"([a-z0-9_]+)"', block)))
    assert {"gemm_tile", "gemm_stages", "s3_tile", "s3_stagger", "s3_min_rows", "no_fold", "s3_m16", "s3_rt", "s3_rt4", "s3_deep4", "s3_w128", "s3_splitk", "attn_pipe", "core_trim", "mlp_fused", "gemm_splitk",
            "attn_m16", "cfg_rows", "vae_lat", "vae_fold", "codec_mfma", "s3_sn", "s3_super4", "s3_super8"} <= set(keys)
    lib = L.lib()
    for k in keys:
        assert lib.avd_tune_set(k.encode(), DEFAULTS[k]) == 0, k
    assert lib.avd_tune_set(b"no_such_knob", 1) == L.EINVAL and b"no_such_knob" in lib.avd_last_error()
    # values outside a key's range are refused and leave the key usable: it takes its default afterwards
    for k, bad in (("s3_rt4", 1), ("s3_rt4", 9), ("s3_splitk", 5), ("s3_splitk", -1), ("gemm_splitk", 5)):
        assert lib.avd_tune_set(k.encode(), bad) == L.EINVAL, (k, bad)
        assert k.encode() in lib.avd_last_error()
        assert lib.avd_tune_set(k.encode(), DEFAULTS[k]) == 0, k


def test_header_symbols_exported_and_bound():
    from multimodal_diffusion_amd import _lib as L
    header = (ROOT / "include" / "avdiff_hip.h").read_text()
    declared = set(re.findall(r"\b(avd_[a-z0-9_]+)\s*\(", header))
    assert len(declared) >= 25
    lib = L.lib()                                  # loads libavdiff_hip.so (no GPU needed to load)
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/avdiff_hip.h but not exported"
        assert name in L.SIGNATURES, f"{name} has no ctypes signature"
    assert set(L.SIGNATURES) <= declared, set(L.SIGNATURES) - declared
    assert lib.avd_abi_version() == L.ABI_VERSION == 7


def test_error_channel_without_gpu():
    from multimodal_diffusion_amd import _lib as L
    lib = L.lib()
    # argument validation happens before any HIP call, so it is testable on a CPU-only box
    assert lib.avd_gemm_bias_act_f32(None, 4, None, None, None, 0, None, 4, 1, 4, 4, 0, None) == L.EINVAL
    assert b"null pointer" in lib.avd_last_error()
    assert lib.avd_attn_fwd_f32(8, 8, 1, 4, 1, 32, 0.1, 4, None, None) == L.EUNSUPPORTED     # head_dim != 64
    with pytest.raises(ValueError):
        L.check(L.EINVAL)
    with pytest.raises(L.AvdError):
        L.check(L.EUNSUPPORTED)
    # bf16x3 entry points: size helpers and shape guards
    assert lib.avd_split3_bytes(300, 512) == 512 * 512 * 6            # rows padded to 256, six bytes per element
    assert lib.avd_split3_bytes(300, 24) == -1                         # K must be a multiple of 16
    assert lib.avd_qkv3_bytes(2, 421, 8) == 3 * 2 * 8 * 448 * 384      # tokens padded to 64, 384-byte rows
    assert lib.avd_qkv3_bytes(0, 421, 8) == -1
    assert lib.avd_gemm_bf16x3_f32(16, 16, None, None, 16, None, 100, 200, 512, 0, 6, None) == L.EUNSUPPORTED   # N % 256 != 0
    assert b"N % 256" in lib.avd_last_error()
    assert lib.avd_gemm_bf16x3_f32(None, 16, None, None, 16, None, 100, 256, 512, 0, 6, None) == L.EINVAL
    assert lib.avd_gemm_bf16x3_f32(16, 16, None, None, 16, None, 100, 256, 512, 0, 7, None) == L.EINVAL                 # terms must be 6, 9 or 1
    assert lib.avd_gemm_bf16x3_qkv3_f32(16, 16, 16, 16, 1000, 421, 8, 512, 0.1, 6, None) == L.EINVAL          # rows not a multiple of tokens
    assert lib.avd_attn_fwd_qkv3_f32(16, 16, None, 2, 421, 8, 500, 6, None) == L.EINVAL                       # n_query > N


def test_schedule_tables_bit_exact_vs_reference():
    from multimodal_diffusion_amd import schedule_utils as su, schedules
    g = load_golden("g1_schedules.npz")
    for kind in ("cosine", "linear", "sigmoid"):
        b = su.make_beta_schedule(1000, kind=kind, min_beta=1e-4, max_beta=0.02)
        al, ab = su.alphas_cumprod_from_betas(b)
        assert np.array_equal(b.numpy(), g[f"betas/{kind}"])
        assert np.array_equal(ab.numpy(), g[f"abar/{kind}"])
        assert torch.equal(al, 1.0 - b)
    for S in (10, 25, 50, 60, 100):
        assert np.array_equal(su.make_sampling_schedule(1000, S).numpy(), g[f"sched/{S}"])
    assert np.array_equal(su.make_sampling_schedule(50, 7).numpy(), g["sched/T50_S7"])
    with pytest.raises(ValueError):
        su.make_beta_schedule(10, kind="bogus")
    sch = schedules.ModalitySchedule.make(kind="cosine", steps=1000)
    assert np.array_equal(sch.alphas_cumprod.numpy(), g["abar/cosine"])
    assert np.array_equal(sch.make_sampling_schedule(25).numpy(), g["sched/25"])
    both = schedules.build_schedules_from_config({"diffusion": {"video": {"steps": 1000}, "audio": {"steps": 50, "schedule": "linear"}}})
    assert both["audio"].steps == 50 and both["video"].kind == "cosine"


def test_state_dict_keys_match_reference(small_model):
    """strict=True loads of the reference's own state dicts (saved in the golden fixture)."""
    import multimodal_diffusion_amd as A
    g, W, meta = small_model
    core = A.MMDiT(d_model=meta["d"], n_layers=meta["n_layers"], n_heads=meta["n_heads"], mlp_ratio=meta["mlp_ratio"])
    core.load_state_dict(W["core"], strict=True)
    head = A.MultiModalNoiseHead({"video": 128, "audio": 128}, {"video": 256, "audio": 32}, hidden_dim=64)
    head.load_state_dict(W["head"], strict=True)
    A.LinearAdapter(256, 64).load_state_dict(W["adapt_v"], strict=True)
    A.LinearAdapter(32, 64).load_state_dict(W["adapt_a"], strict=True)
    full = A.MMDiT(d_model=512, n_layers=8, n_heads=8, mlp_ratio=4.0)
    sd = full.state_dict()
    assert sd["blocks.7.attn.mha.in_proj_weight"].shape == (1536, 512)
    assert sd["blocks.0.mlp.fc1.weight"].shape == (2048, 512) and sd["final_norm.scale"].shape == (512,)
    assert sum(p.numel() for p in full.parameters()) == 25_211_392          # core parameter count
    h = A.MultiModalNoiseHead({"video": 512, "audio": 512}, {"video": 256, "audio": 32}, hidden_dim=512)
    assert sum(p.numel() for p in h.parameters()) == 1_200_416              # head parameter count


def test_head_variants_build():
    import multimodal_diffusion_amd as A
    h = A.MultiModalNoiseHead({"video": 64, "audio": 64}, {"video": 16, "audio": 8}, hidden_dim=32,
                              num_shared_layers=1, num_modality_specific_layers=3)
    keys = set(h.state_dict())
    assert "spec.video.1.0.weight" in keys and "spec.audio.0.1.bias" in keys and "shared.0.0.weight" in keys
    h2 = A.MultiModalNoiseHead({"video": 64}, {"video": 16}, hidden_dim=32, num_shared_layers=0,
                               num_modality_specific_layers=2, share_parameters=True)
    assert "shared_specific_trunk.0.0.weight" in set(h2.state_dict())
    assert len(h2._trunk("video")) == 1 and len(h._trunk("audio")) == 3
    with pytest.raises(ValueError):
        A.MultiModalNoiseHead({"video": 64}, {"video": 16}, activation="tanh")


def test_no_cpu_fallback():
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import _lib as L, ops, schedule_utils as su
    core = A.MMDiT(d_model=128, n_layers=1, n_heads=2, mlp_ratio=2.0).eval()
    with pytest.raises(L.AvdError):
        core(torch.zeros(1, 4, 128))
    with pytest.raises(L.AvdError):
        ops.tube_patch_video(torch.zeros(1, 8, 2, 4, 4), 2, 4, 4)
    with pytest.raises(L.AvdError):
        su.ddim_step(torch.zeros(1, 4), torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.long),
                     torch.zeros(1, 4), torch.ones(10))
    with pytest.raises(L.AvdError):
        A.DenoiseEngine(adapt_v=A.LinearAdapter(256, 64), adapt_a=A.LinearAdapter(32, 64), core=core,
                        head=A.MultiModalNoiseHead({"video": 128, "audio": 128}, {"video": 256, "audio": 32}, hidden_dim=64),
                        tstep_dim=64, target="video", latent_shape=(1, 8, 4, 8, 8), prompt_tokens=5,
                        alpha_bar=torch.ones(10), guidance=1.0)
    ln = A.MMDiT(d_model=128, n_layers=1, n_heads=2, norm="layernorm")          # build_norm's other branch (mmdt.py:44-45)
    assert {"blocks.0.norm1.weight", "blocks.0.norm1.bias", "final_norm.weight", "final_norm.bias"} <= set(ln.state_dict())
    with pytest.raises(L.AvdError):
        ln.eval()(torch.zeros(1, 4, 128))
    # rope=True is accepted and ignored, as in the reference (mmdt.py:125-127 stores the flag and never reads it)
    rp = A.MMDiT(d_model=128, n_layers=1, n_heads=2, rope=True)
    assert rp.cfg.rope is True and set(rp.state_dict()) == set(A.MMDiT(d_model=128, n_layers=1, n_heads=2).state_dict())


def test_product_does_not_import_oracle():
    pkg = ROOT / "multimodal_diffusion_amd"
    for f in pkg.rglob("*.py"):
        src = f.read_text()
        assert "oracle" not in src, f"{f} mentions the oracle: the product path must not depend on it"
    for f in list(pkg.rglob("*.hip")) + list(pkg.rglob("*.h")):
        assert "oracle" not in f.read_text()


def test_chunk_view_and_shard_ranges():
    from multimodal_diffusion_amd import ops, dist as D
    x = torch.arange(2 * 3 * 10, dtype=torch.float32).view(2, 3, 10)
    w = ops.chunk_1d(x, length=4, stride=3)
    assert w.shape == (2, 3, 3, 4) and torch.equal(w[1, 2, 1], x[1, 2, 3:7])
    assert w.data_ptr() == x.data_ptr()                       # a view, like the reference's unfold
    assert ops.chunk_1d(x, length=20, stride=4).shape == (2, 3, 1, 10)
    for B, world in ((32, 1), (256, 8), (10, 4), (3, 8)):
        spans = [D.shard_range(B, r, world) for r in range(world)]
        assert spans[0][0] == 0 and spans[-1][1] == B
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        sizes = [hi - lo for lo, hi in spans]
        assert max(sizes) - min(sizes) <= 1
    with pytest.raises(ValueError):
        D.shard_range(4, 4, 4)


def test_bench_flop_model_matches_survey():
    import bench
    # GFLOP per sample per step (head on target rows only)
    for size, want in ((32, 4.41), (64, 6.35), (128, 14.33), (256, 49.65), (512, 245.3)):
        nv = 6 * (size // 32) ** 2
        got = bench.step_flops_per_sample(nv, 37) / 1e9
        assert abs(got - want) / want < 2e-3, (size, got, want)


def test_bench_plain_run_and_dump_outputs(tmp_path, monkeypatch):
    """bench.py's arguments: --full is off by default and --dump-outputs takes a directory; dump_latent writes float32, keeps whole
    leading samples up to the size cap, and only the leading values of the first sample when one sample alone passes it."""
    import numpy as np
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    a = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"
    z = torch.randn(5, 8, 12, 2, 2)
    bench.dump_latent(str(tmp_path / "out"), z)
    got = np.load(tmp_path / "out" / "latent.npy")
    assert got.dtype == np.float32 and np.array_equal(got, z.numpy())
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 3 * z[0].numel() * 4 + 100)
    bench.dump_latent(str(tmp_path / "out"), z.double())
    got = np.load(tmp_path / "out" / "latent.npy")
    assert got.dtype == np.float32 and np.array_equal(got, z[:3].numpy())
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 40 * 4)
    bench.dump_latent(str(tmp_path / "out"), z)
    assert np.array_equal(np.load(tmp_path / "out" / "latent.npy"), z.reshape(-1)[:40].numpy())


def test_checkpoint_interop(tmp_path, small_model):
    """next-4: both checkpoint layouts of the reference load; the trainer layout reports its embedding mode."""
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import checkpoint as CK
    _, W, meta = small_model

    def fresh(adapter_out):
        core = A.MMDiT(d_model=meta["d"], n_layers=meta["n_layers"], n_heads=meta["n_heads"], mlp_ratio=meta["mlp_ratio"])
        head = A.MultiModalNoiseHead({"video": 128, "audio": 128}, {"video": 256, "audio": 32}, hidden_dim=64)
        return dict(core=core, head=head, adapt_v=A.LinearAdapter(256, adapter_out), adapt_a=A.LinearAdapter(32, adapter_out))

    # (1) sampler layout: {name}_state_dict (sample_clip.py:122-126)
    mods = fresh(64)
    p1 = tmp_path / "sampler.pt"
    torch.save({f"{k}_state_dict": W[k] for k in ("core", "head", "adapt_v", "adapt_a")}, p1)
    CK.load_checkpoint_maybe({"paths": {"ckpt_path": str(p1)}}, mods)
    assert torch.equal(mods["core"].state_dict()["blocks.0.mlp.fc1.weight"], W["core"]["blocks.0.mlp.fc1.weight"])
    CK.load_checkpoint_maybe({"paths": {}}, mods)                                # no path: random weights, no error
    with pytest.raises(FileNotFoundError):
        CK.load_checkpoint_maybe({"paths": {"ckpt_path": str(tmp_path / "nope.pt")}}, mods)

    # (2) trainer layout (trainer.py:407-423): d-wide adapters (add-mode), DDP prefixes, EMA of the core
    mods = fresh(128)
    ema = {k: v * 0.5 for k, v in W["core"].items()}
    tr = {"step": 1234, "core": {f"module.{k}": v for k, v in W["core"].items()}, "head": W["head"],
          "adapt_v": {"proj.weight": torch.randn(128, 256), "proj.bias": torch.zeros(128)},
          "adapt_a": {"proj.weight": torch.randn(128, 32), "proj.bias": torch.zeros(128)}, "opt": {}, "ema": ema}
    p2 = tmp_path / "trainer.pt"
    torch.save(tr, p2)
    info = CK.load_trainer_checkpoint(p2, mods)
    assert info == {"step": 1234, "loaded": ["adapt_v", "adapt_a", "core", "head"], "temb_mode": "add"}
    assert torch.equal(mods["core"].state_dict()["final_norm.scale"], W["core"]["final_norm.scale"])
    CK.load_trainer_checkpoint(p2, mods, use_ema=True)
    assert torch.equal(mods["core"].state_dict()["final_norm.scale"], ema["final_norm.scale"])
    assert CK.load_trainer_checkpoint(tr, fresh(64) | {"adapt_v": None, "adapt_a": None})["temb_mode"] is None


def test_agpr_hazard_lint_on_synthetic_listings(tmp_path):
    """tools/check_agpr_hazards.py (run by build() on the two kernels whose MFMAs are asm statements): an AGPR read one slot behind the
    asm-statement MFMA that wrote it fails the lint; the same read behind the kernels' `s_nop 15` pair passes; an MFMA the compiler
    emitted itself (outside ASMSTART / ASMEND: its hazard recogniser pads it) is not counted — and a listing with NO asm-statement MFMA at all
    is refused (round 5, ADVICE r4: the files handed to the lint are expected to hold such MFMAs; finding none means it looked at nothing)."""
    import subprocess
    import sys
    tool = str(ROOT / "tools" / "check_agpr_hazards.py")
    head = "_ZN3avd4testEv:\n"
    mfma = "\t;;#ASMSTART\n\tv_mfma_f32_16x16x32_bf16 a[4:7], v[0:3], v[4:7], a[4:7]\n\t;;#ASMEND\n"
    bad = head + mfma + "\tv_accvgpr_read_b32 v9, a5\n"
    good = head + mfma.replace("a[4:7]\n\t;;#ASMEND", "a[4:7]\n\ts_nop 15\n\ts_nop 15\n\t;;#ASMEND") + "\tv_accvgpr_read_b32 v9, a5\n"
    own = head + "\tv_mfma_f32_16x16x32_bf16 a[4:7], v[0:3], v[4:7], a[4:7]\n\tv_accvgpr_read_b32 v9, a5\n"
    other = head + mfma + "\tv_accvgpr_read_b32 v9, a9\n"          # a different register: no dependence
    for name, text, rc, word in (("bad", bad, 1, "FAIL"), ("good", good, 0, "ok"), ("own", own, 2, "nothing to check"), ("other", other, 0, "")):
        f = tmp_path / f"{name}.s"
        f.write_text(text)
        r = subprocess.run([sys.executable, tool, str(f)], capture_output=True, text=True)
        assert r.returncode == rc, (name, r.stdout, r.stderr)
        assert word in r.stdout, (name, r.stdout)


def _s3_supertile(tile, nbn, s3_sn=0, super4=0, super8=0):
    """mirror of s3_supertile (csrc/gemm_bf16x3.hip): (sn, sm) of the two-per-CU (tile) / one-per-CU kernels"""
    sn = 8
    while nbn % sn:
        sn >>= 1
    if tile and nbn <= 16:
        sn = nbn
    total = 32 if tile else 16
    if tile and nbn >= 8 and nbn % 4 == 0:
        sn, total = 4, 64
    if s3_sn > 0:
        sn = min(s3_sn, nbn)
        while nbn % sn:
            sn -= 1
    override = super4 if tile else super8
    if override > 0:
        total = override
    return sn, max(total // sn, 1)


def _s3_block_of(b, nwg, nbm, nbn, sm, sn):
    """mirror of s3_block_of (csrc/s3_common.h): block id -> (block row, block column)"""
    q, r, x = nwg >> 3, nwg & 7, b & 7
    wg = (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + (b >> 3)
    per_row = sm * nbn
    srow, rem = divmod(wg, per_row)
    h = min(nbm - srow * sm, sm)
    sc, rem2 = divmod(rem, h * sn)
    return srow * sm + rem2 // sn, sc * sn + rem2 % sn


def test_s3_block_map_is_a_bijection():
    """The split GEMMs' block-to-tile map (XCD remap, then super-tiles with a ragged last super-row) sends the nbm x nbn block ids onto
    the block grid one to one — for the default super-tile shapes and for the "s3_sn" / "s3_super4" / "s3_super8" values that
    tests/test_gpu_kernel_variants.py sets, on both kernel families.  Host arithmetic only."""
    keys = [(0, 0), (2, 8), (3, 6), (4, 4), (1, 3), (2, 1)]          # (s3_sn, s3_super4 resp. s3_super8)
    for tile in (False, True):
        for s3_sn, total in keys:
            for nbn in range(1, 17):
                sn, sm = _s3_supertile(tile, nbn, s3_sn, total, total)
                assert sn >= 1 and sm >= 1 and nbn % sn == 0, (tile, s3_sn, total, nbn)
                for nbm in (1, 2, 3, 5, 11, 17, 33):
                    nwg = nbm * nbn
                    seen = {_s3_block_of(b, nwg, nbm, nbn, sm, sn) for b in range(nwg)}
                    assert seen == {(i, j) for i in range(nbm) for j in range(nbn)}, (tile, s3_sn, total, nbn, nbm)
    # the five settings of the GPU test give the super-tiles its table names (11 block rows)
    assert _s3_supertile(True, 4, 2, super4=8) == (2, 4) and _s3_supertile(True, 12, 3, super4=6) == (3, 2)
    assert _s3_supertile(True, 12, 4, super4=4) == (4, 1) and _s3_supertile(False, 2, 1, super8=3) == (1, 3)
    assert _s3_supertile(False, 6, 2, super8=1) == (2, 1)
