"""Worker of tests/test_gpu_seeded_noise.py::test_stream_generate_seeded_eta_sharded_two_ranks_share_device: the twin of
tests/_stream_shard_worker.py with stochastic DDIM (ddim_eta 0.5) and the seeded noise stream (noise_seed).  `stream_generate(shard=True)`
under `python -m torch.distributed.run --nproc-per-node 2` with gloo, both ranks on cuda:0, in both directions (audio prompt -> uint8
video, video prompt -> waveform); rank 0 then runs the same generations in one process, once with the default batching and once with
max_windows_per_batch=1, and writes whether the stitched results are bit-identical."""
import json
import os
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import multimodal_diffusion_amd as A  # noqa: E402
from multimodal_diffusion_amd import dist as D, stream_infer as S  # noqa: E402
from oracle import ref_cpu as R  # noqa: E402  (seeded weight recipe only: test infrastructure)

rank, world, _ = D.init_from_env("gloo")
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)

ws = R.synth_weights(seed=3, n_layers=2)
core = A.MMDiT(d_model=512, n_layers=2, n_heads=8, mlp_ratio=4.0).eval()
core.load_state_dict(ws["core"], strict=True)
head = A.MultiModalNoiseHead({"video": 512, "audio": 512}, {"video": 256, "audio": 32}, hidden_dim=512).eval()
head.load_state_dict(ws["head"], strict=True)
av, aa = A.LinearAdapter(256, 256), A.LinearAdapter(32, 256)
av.load_state_dict(ws["adapt_v"])
aa.load_state_dict(ws["adapt_a"])
core, head, av, aa = (m.to(dev) for m in (core, head, av, aa))
core.matmul = head.matmul = "f32"          # one kernel family whatever the shard size (the "auto" rule switches at 2,048 / 6,144 rows)
torch.manual_seed(8)                       # identical codec / VAE weights on both ranks
vae = A.VideoVAE.from_config({"latent": {"channels": 8, "t_down": 4, "s_down": 8}}).eval().to(dev)
codec = A.AudioCodec.from_config({"sr": 16000, "latent": {"channels": 8, "frames_per_clip": 150}, "codec": {"hop_samples": 320}}).eval().to(dev)
cfg = {"tokenizer": {"width": 512, "video": {"tube": {"t": 2, "h": 4, "w": 4}}, "audio": {"chunk": {"length": 4, "stride": 4}}},
       "video": {"fps": 16, "size": [32, 32], "latent": {"channels": 8, "t_down": 4, "s_down": 8}},
       "audio": {"sr": 16000, "latent": {"channels": 8, "frames_per_clip": 150}},
       "data": {"clip_seconds": 0.5}, "streaming": {"window_seconds": 0.5, "hop_seconds": 0.25, "crossfade_seconds": 0.125},
       "diffusion": {m: {"steps": 1000, "sampler_steps": 3, "schedule": "cosine", "min_beta": 1e-4, "max_beta": 0.02} for m in ("video", "audio")},
       "sampling": {"ddim_eta": 0.5, "guidance_scale": {"video": 2.0, "audio": 2.0}}}
wav = (0.1 * torch.randn(18000, generator=torch.Generator().manual_seed(9))).numpy()      # 4 windows of 0.5 s at a 0.25 s hop
kw = dict(cfg=cfg, vid_vae=vae, aud_codec=codec, adapt_v=av, adapt_a=aa, core=core, head=head, tstep_dim=256, device=dev,
          prompt_modality="audio", prompt_video=None, prompt_audio=wav, seed=10, noise_seed=0x5EEDF00D00000013)
n_win = S.split_audio_into_windows(wav, sr=16000, win_s=0.5, hop_s=0.25)[0].shape[0]

sharded = S.stream_generate(shard=True, **kw)
vid = torch.randint(0, 256, (12, 32, 32, 3), generator=torch.Generator().manual_seed(11), dtype=torch.uint8).numpy()
kw_a = dict(kw, prompt_modality="video", prompt_video=vid, prompt_audio=None, seed=12)
n_win_a = S.split_frames_into_windows(vid, fps=16, win_s=0.5, hop_s=0.25)[0].shape[0]
sharded_a = S.stream_generate(shard=True, **kw_a)
D.barrier()
torch.distributed.destroy_process_group()
if rank == 0:
    single = S.stream_generate(shard=False, **kw)
    single_a = S.stream_generate(shard=False, **kw_a)
    per_window = S.stream_generate(shard=False, max_windows_per_batch=1, **kw)
    per_window_a = S.stream_generate(shard=False, max_windows_per_batch=1, **kw_a)
    other_seed = S.stream_generate(shard=False, **dict(kw, noise_seed=1))
    Path(os.environ["AVD_TEST_OUT"]).write_text(json.dumps({
        "world": world, "windows": int(n_win), "audio_windows": int(n_win_a),
        "video_sharded_equal": bool(sharded is not None and np.array_equal(sharded["video"], single["video"])),
        "video_per_window_equal": bool(np.array_equal(per_window["video"], single["video"])),
        "audio_sharded_equal": bool(sharded_a is not None and np.array_equal(sharded_a["audio"], single_a["audio"])),
        "audio_per_window_equal": bool(np.array_equal(per_window_a["audio"], single_a["audio"])),
        "eta_changes_result": bool(not np.array_equal(other_seed["video"], single["video"]))}))
