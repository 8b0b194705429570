"""CPU-only checks of what the two pipelines share (no GPU, no module, no kernel launch): sample_one_direction and stream_generate
refuse the same faulty calls with the same words before they touch a device, and schedule_utils.trajectory_segments is
guidance_segments on a schedule without jumps and step_segments on a resampling schedule."""
import numpy as np
import pytest
import torch

from _kit import STREAM_HALF_SECOND, pipeline_cfg

WAV = np.zeros(18000, dtype=np.float32)                                     # 4 windows of 0.5 s
VID = np.zeros((20, 32, 32, 3), dtype=np.uint8)                             # 4 windows of 0.5 s
MASK = torch.ones(8, 1, 4, 4)                                               # never looked at: every fault below comes first
A2V = dict(prompt_modality="audio", prompt_video=None, prompt_audio=WAV)
V2A = dict(prompt_modality="video", prompt_video=VID, prompt_audio=None)

# (what is wrong, the direction, the faulty arguments, what the message must say)
FAULTS = [
    ("both init clips", A2V, dict(init_video=VID, init_audio=WAV), ["not both"]),
    ("a mask without an init clip", A2V, dict(mask=MASK), ["init clip"]),
    ("strength 0.5 without an init clip", A2V, dict(strength=0.5), ["init clip", "strength"]),
    ("strength -0.1", A2V, dict(init_video=VID, strength=-0.1), ["strength"]),
    ("strength 1.5", A2V, dict(init_video=VID, strength=1.5), ["strength"]),
    ("init_audio on audio->video", A2V, dict(init_audio=WAV), ["init_audio"]),
    ("init_video on video->audio", V2A, dict(init_video=VID), ["init_video"]),
    ("a float32 init_video", A2V, dict(init_video=VID.astype(np.float32)), ["init_video", "uint8"]),
    ("an int16 init_audio", V2A, dict(init_audio=WAV.astype(np.int16)), ["init_audio", "waveform"]),
    ("resample without a mask", A2V, dict(init_video=VID, resample=(2, 2), noise_seed=1), ["needs an init clip with a mask"]),
    ("resample without noise_seed", A2V, dict(init_video=VID, mask=MASK, resample=(2, 2)), ["noise_seed"]),
]


@pytest.mark.parametrize("what, direction, faulty, words", FAULTS, ids=[f[0] for f in FAULTS])
def test_both_pipelines_refuse_with_the_same_words(what, direction, faulty, words):
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import stream_infer as S
    mods = dict(vid_vae=None, aud_codec=None, adapt_v=None, adapt_a=None, core=None, head=None, tstep_dim=256, device=torch.device("cpu"))
    cfg = pipeline_cfg(clip_seconds=0.5, sampler_steps=4, streaming=STREAM_HALF_SECOND)
    said = []
    for fn in (A.sample_one_direction, S.stream_generate):
        with pytest.raises(ValueError) as err:
            fn(cfg=cfg, **mods, **direction, **faulty)
        said.append(str(err.value))
    assert said[0] == said[1]
    for w in words:
        assert w in said[0], (what, said[0])


def test_trajectory_segments():
    from multimodal_diffusion_amd import schedule_utils as su
    plain = su.make_sampling_schedule(1000, 8)
    climb = torch.tensor([990, 900, 360, 700, 650, -1])          # an up-pair to a timestep not seen before: still a denoising step
    equal = torch.tensor([999, 749, 749, -1])                    # equal neighbours: legal without jumps
    for s in (plain, climb, equal, torch.tensor([-1]), torch.tensor([999, -1])):
        assert not su.has_jumps(s)
        for iv in (None, (300, 800), (0, 0), (700, 999)):
            assert su.trajectory_segments(s, iv) == [(a, b, "cfg" if c else "cond") for a, b, c in su.guidance_segments(s, iv)]
    assert su.trajectory_segments(plain, None) == [(0, 8, "cfg")]
    assert su.trajectory_segments(plain, (300, 800)) == [(0, 2, "cond"), (2, 6, "cfg"), (6, 8, "cond")]
    assert su.trajectory_segments(climb, None) == [(0, 5, "cfg")] and su.trajectory_segments(equal, None) == [(0, 3, "cfg")]
    assert su.trajectory_segments(torch.tensor([-1]), None) == []
    r = su.resample_schedule(su.make_sampling_schedule(1000, 4), 2, 2)
    assert su.has_jumps(r)
    for iv in (None, (300, 800), (499, 499)):
        assert su.trajectory_segments(r, iv) == su.step_segments(r, iv)
    assert su.trajectory_segments(r, None) == [(0, 2, "cfg"), (2, 3, "renoise"), (3, 7, "cfg")]
    with pytest.raises(ValueError, match="both 749"):            # on a resampling schedule equal neighbours stay refused
        su.trajectory_segments(torch.tensor([999, 749, 749, 999, 749, -1]), None)
