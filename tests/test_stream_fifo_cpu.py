"""CPU tests of ``stream_generate(sampler="fifo")`` and of the guided FIFO queue shift: ``fifo_geometry`` on hand-computed cases,
every refusal of the new path raised before an encoder is touched, the old path taken call for call under ``sampler`` None /
"windows", and every refusal ``avd_fifo_shift_guided_f32`` makes before a launch."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from _kit import STREAM_HALF_SECOND, audio_prompt, pipeline_cfg, video_prompt, with_sampling

ROOT = Path(__file__).resolve().parent.parent
STREAM_ONE_SECOND = {"window_seconds": 1.0, "hop_seconds": 0.5, "crossfade_seconds": 0.25}


def shipped_cfg(**tokenizer):
    """the reference's shipped geometry: 3 s windows every 1 s, 16 fps over t_down 4 (12 latent frames), 150 audio latent frames,
    tube t = 2, chunk 4 / 4"""
    return pipeline_cfg(clip_seconds=3.0, sampler_steps=50, size=(256, 256), streaming={"window_seconds": 3.0, "hop_seconds": 1.0},
                        tokenizer=tokenizer or None)


# ------------------------------------------------------------------------------------------------- geometry
def test_geometry_of_the_reduced_configs():
    from multimodal_diffusion_amd.stream_infer import fifo_geometry
    g = fifo_geometry(pipeline_cfg(clip_seconds=1.0, sampler_steps=4, streaming=STREAM_ONE_SECOND), "audio", 4, 4)
    assert (g.S, g.slot_len, g.B, g.prompt_hop, g.P, g.n_slots, g.P_p) == (2, 2, 2, 75, 10, 5, 375)
    assert (g.hop_t, g.L_t, g.hop_p, g.L_p, g.h) == (2, 4, 75, 150, 2)
    g = fifo_geometry(pipeline_cfg(clip_seconds=0.5, sampler_steps=4, streaming=STREAM_HALF_SECOND), "audio", 4, 4)
    assert (g.S, g.B, g.P, g.n_slots) == (1, 4, 5, 3)                            # 3 slots of 2 = 6 positions: the canvas is cropped to 5
    assert (g.slot_len, g.prompt_hop, g.hop_t, g.L_t) == (2, 150, 1, 2)


def test_geometry_of_the_shipped_config():
    from multimodal_diffusion_amd.stream_infer import fifo_geometry
    cfg = shipped_cfg()
    with pytest.raises(ValueError, match=r"50 steps.*48 and 54"):
        fifo_geometry(cfg, "audio", 3, 50)
    g = fifo_geometry(cfg, "audio", 3, 48)
    assert (g.S, g.slot_len, g.prompt_hop, g.B, g.h) == (6, 2, 25, 8, 6)
    assert (g.P, g.n_slots, g.P_p) == (2 * 4 + 12, 10, 2 * 50 + 150)
    g = fifo_geometry(cfg, "audio", 3, 48, lookahead=3)
    assert (g.h, g.B) == (3, 16)
    with pytest.raises(ValueError, match=r"lookahead 6 must be below the S = 6"):
        fifo_geometry(cfg, "audio", 3, 48, lookahead=6)
    # video -> audio: 150 latent frames in slots of 4 are S = 37 (148 positions); 12 * 4 / 150 prompt positions per slot is refused
    with pytest.raises(ValueError, match=r"the prompt has 0\.32 latent positions per target slot.*whole positions"):
        fifo_geometry(cfg, "video", 3, 37)
    with pytest.raises(ValueError, match=r"length 4 and stride 2.*non-overlapping"):
        fifo_geometry(shipped_cfg(audio={"chunk": {"length": 4, "stride": 2}}), "video", 3, 37)
    for bad in (dict(n_windows=0), dict(steps=0), dict(lookahead=-1), dict(steps=True)):
        with pytest.raises(ValueError, match="must be an int"):
            fifo_geometry(cfg, "audio", **dict(dict(n_windows=3, steps=48), **bad))


def test_geometry_of_a_dividing_video_prompt():
    from multimodal_diffusion_amd.stream_infer import fifo_geometry
    cfg = pipeline_cfg(clip_seconds=1.0, sampler_steps=4, streaming=STREAM_ONE_SECOND)
    cfg["audio"]["latent"]["frames_per_clip"] = 16
    g = fifo_geometry(cfg, "video", 4, 4)
    assert (g.S, g.slot_len, g.prompt_hop, g.B, g.hop_t, g.L_t, g.hop_p, g.L_p) == (4, 4, 1, 1, 8, 16, 2, 4)
    assert (g.P, g.n_slots, g.P_p) == (40, 10, 10)


# ------------------------------------------------------------------------------------------------- refusals before any encoder
class Touched(Exception):
    pass


class Boom:
    """a VAE / codec that no refusal may reach"""

    def encode(self, x):
        raise Touched("encode")

    def decode(self, z):
        raise Touched("decode")


def _kw(cfg, prompt):
    return dict(cfg=cfg, vid_vae=Boom(), aud_codec=Boom(), adapt_v=None, adapt_a=None, core=None, head=None, tstep_dim=256,
                device=torch.device("cpu"), **prompt)


def _one_second_prompts():
    wav = np.zeros(36000, dtype=np.float32)                                      # 4 windows of 1.0 s every 0.5 s
    vid = np.zeros((40, 32, 32, 3), dtype=np.uint8)
    return (dict(prompt_modality="audio", prompt_video=None, prompt_audio=wav), dict(prompt_modality="video", prompt_video=vid,
                                                                                     prompt_audio=None))


def test_fifo_refusals_come_before_any_encoder():
    from multimodal_diffusion_amd import stream_infer as S
    cfg = pipeline_cfg(clip_seconds=1.0, sampler_steps=4, streaming=STREAM_ONE_SECOND)
    a2v, v2a = _one_second_prompts()
    kw = _kw(cfg, a2v)
    init = dict(init_video=np.zeros((40, 32, 32, 3), dtype=np.uint8), mask=torch.ones(8, 10, 4, 4))
    for args, match in ((dict(shard=True), "shard=True"),
                        (dict(consensus="uniform"), "no consensus"),
                        (dict(noise_keying="canvas", noise_seed=1), "noise_keying='canvas'"),
                        (dict(resample=(2, 2), noise_seed=1, **init), "no resample"),
                        (dict(init_noise=torch.zeros(4, 8, 4, 4, 4)), "no init_noise"),
                        (dict(fifo={"step": 4}), "steps, lookahead and graph"),
                        (dict(fifo={"steps": 0}), r"fifo\['steps'\]"),
                        (dict(fifo={"lookahead": -1}), r"fifo\['lookahead'\]"),
                        (dict(fifo={"graph": 1}), r"fifo\['graph'\]"),
                        (dict(fifo={"steps": 5}), r"5 steps.*4 and 6"),
                        (dict(fifo={"lookahead": 2}), "lookahead 2 must be below"),
                        (dict(strength=0.5, fifo={"steps": 6}, **init), r"3 steps.*2 and 4")):      # the truncated length must divide
        with pytest.raises(ValueError, match=match):
            S.stream_generate(sampler="fifo", **dict(kw, **args))
    # the config's own settings are refused like the arguments
    for streaming, match in (({"latent_consensus": "uniform"}, "no consensus"), ({"noise_keying": "canvas"}, "noise_keying='canvas'"),
                             ({"fifo": {"window": 1}}, "steps, lookahead and graph")):
        with pytest.raises(ValueError, match=match):
            S.stream_generate(sampler="fifo", **dict(kw, cfg=dict(cfg, streaming=dict(STREAM_ONE_SECOND, **streaming))))
    with pytest.raises(ValueError, match="no resample"):
        S.stream_generate(sampler="fifo", **dict(kw, cfg=with_sampling(cfg, resample={"jump": 2, "resamples": 2})))
    with pytest.raises(ValueError, match=r"momentum 0\.5.*no slot momentum"):
        S.stream_generate(sampler="fifo", **dict(kw, cfg=with_sampling(cfg, apg={"video": {"norm_threshold": 2.0, "momentum": 0.5}})))
    # video -> audio at the reduced geometry: 4 * 4 / 150 prompt positions per slot; overlapping chunks
    with pytest.raises(ValueError, match="whole positions"):
        S.stream_generate(sampler="fifo", **_kw(cfg, v2a))
    lapped = pipeline_cfg(clip_seconds=1.0, sampler_steps=4, streaming=STREAM_ONE_SECOND,
                          tokenizer={"audio": {"chunk": {"length": 4, "stride": 2}}})
    with pytest.raises(ValueError, match="non-overlapping"):
        S.stream_generate(sampler="fifo", **_kw(lapped, v2a))
    with pytest.raises(ValueError, match=r"sampler must be one of \('windows', 'fifo'\)"):
        S.stream_generate(sampler="diagonal", **kw)
    with pytest.raises(ValueError, match="sampler must be one of"):
        S.stream_generate(**dict(kw, cfg=dict(cfg, streaming=dict(STREAM_ONE_SECOND, sampler="queue"))))
    # data.clip_seconds must give the window's latent length: the decode runs on windows
    with pytest.raises(ValueError, match="they must be equal"):
        S.stream_generate(sampler="fifo", **dict(kw, cfg=dict(cfg, data={"clip_seconds": 2.0})))


def test_windows_and_none_take_the_old_path(monkeypatch):
    from multimodal_diffusion_amd import stream_infer as S
    cfg = pipeline_cfg(clip_seconds=0.5, sampler_steps=4, streaming=STREAM_HALF_SECOND)
    kw = _kw(cfg, {k: v for k, v in audio_prompt().items()})
    entered = []

    def fifo_path(*a, **k):
        entered.append(k)
        raise Touched("fifo")

    monkeypatch.setattr(S, "_stream_generate_fifo", fifo_path)
    for sampler in (None, "windows"):
        with pytest.raises(Touched, match="encode"):                             # today's path: straight to the prompt encoder
            S.stream_generate(sampler=sampler, fifo={"nothing": "reads this"}, **kw)
    assert not entered
    with pytest.raises(Touched, match="encode"):
        S.stream_generate(**kw)                                                  # as every existing caller writes it
    assert not entered
    with pytest.raises(Touched, match="fifo"):
        S.stream_generate(sampler="fifo", **kw)
    with pytest.raises(Touched, match="fifo"):                                   # streaming.sampler selects it, the argument wins
        S.stream_generate(**dict(kw, cfg=dict(cfg, streaming=dict(STREAM_HALF_SECOND, sampler="fifo"))))
    assert len(entered) == 2 and entered[0]["seed"] == 10
    with pytest.raises(Touched, match="encode"):
        S.stream_generate(sampler="windows", **dict(kw, cfg=dict(cfg, streaming=dict(STREAM_HALF_SECOND, sampler="fifo"))))
    sig = inspect.signature(S.stream_generate).parameters
    assert sig["sampler"].default is None and sig["fifo"].default is None


def test_a_video_prompt_reaches_the_shared_split():
    """the helpers both samplers share give the old path's shapes: a video prompt's windows and the audio target's latent"""
    from multimodal_diffusion_amd import _pipeline as P
    from multimodal_diffusion_amd import stream_infer as S
    cfg = pipeline_cfg(clip_seconds=0.5, sampler_steps=4, streaming=STREAM_HALF_SECOND)
    pc = P.read_config(cfg, "video", guidance_interval=None, resample=None, has_init=False, has_mask=False, noise_seed=None)
    chunks, zp_shape, lat = S._prompt_windows(cfg, pc, "video", video_prompt()["prompt_video"], None)
    assert chunks.shape == (4, 8, 32, 32, 3) and zp_shape == (4, 8, 2, 4, 4) and lat == (8, 150)
    with pytest.raises(ValueError, match="2 windows, the prompt into 4"):
        S._init_windows(cfg, pc, np.zeros(12000, dtype=np.float32), 4)
    mc = S._canvas_mask(torch.ones(1), lat, 4, 75, 150)
    assert tuple(mc.shape) == (8, 375)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        S._canvas_mask(torch.full((1,), 2.0), lat, 4, 75, 150)


def test_fifo_denoise_takes_guided_shift_with_an_init_canvas_only():
    import multimodal_diffusion_amd as A
    eng = object.__new__(A.DenoiseEngine)
    eng.latent_shape, eng.device, eng.target, eng.tube, eng._clip = (2, 8, 4, 16, 16), torch.device("cpu"), "video", (2, 4, 4), None
    args = (eng, torch.zeros(8, 40), 20, torch.tensor([999, 749, 499, 249, -1]), 3, 1)
    with pytest.raises(ValueError, match="guided_shift"):
        A.fifo_denoise(*args, guided_shift=True)
    with pytest.raises(ValueError, match="guided_shift"):
        A.fifo_denoise(*args, init_canvas=torch.randn(8, 10, 16, 16), guided_shift=1)
    assert inspect.signature(A.fifo_denoise).parameters["guided_shift"].default is False


# ------------------------------------------------------------------------------------------------- the C entry
P0, BIG = 4096, 1 << 30                             # non-null, 16-byte aligned stand-ins: nothing is dereferenced


def _guide(**kw):
    from multimodal_diffusion_amd import _lib as L
    f = dict(known=5 * BIG, mask=None, P=64, seed=4321, first=0, stride=2, cursor=None)
    f.update(kw)
    return L.ClipGuide(f["known"], f["mask"], f["P"], f["seed"], f["first"], f["stride"], f["cursor"])


def test_header_and_bindings_name_the_guided_shift():
    from multimodal_diffusion_amd import _lib as L
    from multimodal_diffusion_amd import functional as Fn
    import multimodal_diffusion_amd as A
    header = (ROOT / "include" / "avdiff_hip.h").read_text()
    assert set(re.findall(r"\b(avd_[a-z0-9_]+)\s*\(", header)) == set(L.SIGNATURES)
    assert "avd_fifo_shift_guided_f32" in L.SIGNATURES and hasattr(L.lib(), "avd_fifo_shift_guided_f32")
    assert L.lib().avd_abi_version() == L.ABI_VERSION == 7                       # an addition: the ABI stays
    assert "Guided FIFO queue shift (a public contract)" in header
    assert "guide" in inspect.signature(Fn.fifo_shift).parameters
    assert "guided" in inspect.signature(A.DenoiseEngine.fifo_shift).parameters


def test_guided_shift_refuses_before_any_launch():
    from multimodal_diffusion_amd import _lib as L
    lib = L.lib()
    key = L.NoiseKey(7, 0)

    def run(g, t=500, c=3, abar=P0, T_train=1000, z_in=2 * BIG, z_out=3 * BIG, popped=4 * BIG, hist_in=None, hist_out=None, B=2,
            outer=8, slots=2, slot_len=2, inner=256, k=key):
        return lib.avd_fifo_shift_guided_f32(None if k is None else C.byref(k), t, c, None if g is None else C.byref(g), abar, T_train,
                                             0, z_in, z_out, popped, hist_in, hist_out, B, outer, slots, slot_len, inner, None)

    assert run(None) == L.EINVAL and b"null clip guide" in lib.avd_last_error()
    assert run(_guide(known=None)) == L.EINVAL and b"null known" in lib.avd_last_error()
    for P in (0, -1, 2 ** 32 + 1):
        assert run(_guide(P=P)) == L.EINVAL and b"[1, 2^32]" in lib.avd_last_error(), P
    assert run(_guide(), abar=None) == L.EINVAL and b"alpha_bar" in lib.avd_last_error()
    assert run(_guide(), T_train=0) == L.EINVAL and b"T_train" in lib.avd_last_error()
    # known / mask over any output: z_out, hist_out, popped
    n = 2 * 8 * 4 * 256 * 4                                                      # the batch's bytes
    assert run(_guide(known=3 * BIG + n - 4)) == L.EINVAL and b"overlap" in lib.avd_last_error()
    assert run(_guide(mask=3 * BIG + 64)) == L.EINVAL and b"overlap" in lib.avd_last_error()
    assert run(_guide(known=7 * BIG + 64), hist_in=6 * BIG, hist_out=7 * BIG) == L.EINVAL and b"overlap" in lib.avd_last_error()
    assert run(_guide(known=4 * BIG + 64)) == L.EINVAL and b"overlap popped" in lib.avd_last_error()
    assert run(_guide(mask=4 * BIG + n // 4 - 4)) == L.EINVAL and b"overlap popped" in lib.avd_last_error()      # popped's last float
    # a history pair given half
    assert run(_guide(), hist_in=6 * BIG) == L.EINVAL and b"go together" in lib.avd_last_error()
    assert run(_guide(), hist_out=7 * BIG) == L.EINVAL and b"go together" in lib.avd_last_error()
    # the shift's own checks still hold
    assert run(_guide(), k=None) == L.EINVAL and b"null noise key" in lib.avd_last_error()
    assert run(_guide(), z_out=2 * BIG + 64) == L.EINVAL and b"z_out must not overlap z_in" in lib.avd_last_error()
    assert run(_guide(), t=-1) == L.EINVAL and run(_guide(), c=-1) == L.EINVAL
    assert run(_guide(), c=2 ** 31) == L.EINVAL and b"2^32" in lib.avd_last_error()
    # first / stride / cursor are not read: values the other entries refuse pass the checks here (the launch itself is not made on a
    # machine without a device, so only the order of the refusals is observed: a bad P still comes first)
    assert run(_guide(stride=0, first=2 ** 40, P=0)) == L.EINVAL and b"[1, 2^32]" in lib.avd_last_error()
