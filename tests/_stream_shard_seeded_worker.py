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
from multimodal_diffusion_amd import dist as D, stream_infer as S  # noqa: E402
from oracle import ref_cpu as R  # noqa: E402  (seeded weight recipe only: test infrastructure)
from _kit import STREAM_HALF_SECOND, audio_prompt, components, modules, pipeline  # noqa: E402

rank, world, _ = D.init_from_env("gloo")
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)

mods = modules(dev, R.synth_weights(seed=3, n_layers=2), 2)
mods[0].matmul = mods[1].matmul = "f32"    # one kernel family whatever the shard size (the "auto" rule switches at 2,048 / 6,144 rows)
vae, codec, cfg = pipeline(dev, seed=8, clip_seconds=0.5, sampler_steps=3, streaming=STREAM_HALF_SECOND,      # the seed: identical
                           sampling={"ddim_eta": 0.5})                                                      # weights on both ranks
kw = dict(components(mods, vae, codec, dev), cfg=cfg, **audio_prompt(), noise_seed=0x5EEDF00D00000013)      # 4 windows of 0.5 s at a 0.25 s hop
wav = kw["prompt_audio"]
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
