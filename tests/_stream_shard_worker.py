"""Worker of tests/test_dist_gloo.py::test_stream_generate_sharded_two_ranks_share_device: `stream_generate(shard=True)` under
`python -m torch.distributed.run --nproc-per-node 2` with gloo, both ranks on cuda:0 — each rank steps AND decodes its own windows,
one gather of the decoded windows to rank 0 — in both directions (audio prompt -> uint8 video, video prompt -> waveform); rank 0 then
runs the same generations in one process and writes whether the stitched results are bit-identical."""
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
                           sampling={"ddim_eta": 0.0})                                                      # weights on both ranks
kw = dict(components(mods, vae, codec, dev), cfg=cfg, **audio_prompt())      # 4 windows of 0.5 s at a 0.25 s hop
wav = kw["prompt_audio"]
n_win = S.split_audio_into_windows(wav, sr=16000, win_s=0.5, hop_s=0.25)[0].shape[0]

sharded = S.stream_generate(shard=True, **kw)
# the V -> A twin: 12 frames at 16 fps = 0.75 s -> windows of 8 frames at a hop of 4: two windows (one per rank), audio out
vid = torch.randint(0, 256, (12, 32, 32, 3), generator=torch.Generator().manual_seed(11), dtype=torch.uint8).numpy()
kw_a = dict(kw, prompt_modality="video", prompt_video=vid, prompt_audio=None, seed=12)
n_win_a = S.split_frames_into_windows(vid, fps=16, win_s=0.5, hop_s=0.25)[0].shape[0]
sharded_a = S.stream_generate(shard=True, **kw_a)
none_elsewhere = D.gather_scalars(1.0 if (sharded is None and sharded_a is None) else 0.0, torch.device("cpu"))
D.barrier()
torch.distributed.destroy_process_group()
if rank == 0:
    single = S.stream_generate(shard=False, **kw)
    single_a = S.stream_generate(shard=False, **kw_a)
    same = sharded is not None and sharded["video"].dtype == np.uint8 and np.array_equal(sharded["video"], single["video"])
    same_a = sharded_a is not None and sharded_a["audio"].dtype == np.float32 and np.array_equal(sharded_a["audio"], single_a["audio"])
    Path(os.environ["AVD_TEST_OUT"]).write_text(json.dumps({
        "world": world, "windows": int(n_win), "shards": [list(D.shard_range(n_win, r, world)) for r in range(world)],
        "rank1_returned_none": none_elsewhere == [0.0, 1.0], "frames_shape": list(single["video"].shape),
        "bit_identical": bool(same), "max_abs_diff": int(np.abs(sharded["video"].astype(np.int32) - single["video"].astype(np.int32)).max()),
        "audio_windows": int(n_win_a), "audio_len": int(single_a["audio"].shape[0]), "audio_bit_identical": bool(same_a),
        "audio_finite_nonzero": bool(np.isfinite(single_a["audio"]).all() and np.abs(single_a["audio"]).max() > 0)}))
