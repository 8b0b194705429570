"""The shared scaffolding of the tests: the device fixture, the reduced (2-layer) and full (8-layer) width-512 model, the DenoiseEngine
builder, the small latent / prompt cases, and the reduced end-to-end pipeline (VideoVAE, AudioCodec and the config dictionary).  Test
modules import from here the way they import `cfg_rows` from `_tune`; a module that imports the `model` or `full` fixture imports `dev`
as well (pytest resolves a fixture's own dependencies in the requesting module).  Nothing here touches the GPU at import time, and the
package is imported inside the functions, so the CPU tests and the shard workers can use `pipeline_cfg`."""
from contextlib import contextmanager

import pytest
import torch

from oracle import ref_cpu as R

ABAR = R.alpha_bar_table(R.beta_table(1000))
# 0.5 s windows every 0.25 s: the streaming block of most stream_generate tests
STREAM_HALF_SECOND = {"window_seconds": 0.5, "hop_seconds": 0.25, "crossfade_seconds": 0.125}


# ------------------------------------------------------------------------------------------------- device and model
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import multimodal_diffusion_amd._lib as L
    buf = (__import__("ctypes").c_char * 64)()
    L.check(L.lib().avd_device_arch(buf, 64))
    assert buf.value.decode().startswith("gfx950"), buf.value
    return torch.device("cuda:0")


def modules(dev, ws, n_layers):
    """(core, head, av, aa) at the model width of mvp.yaml (d = 512, 8 heads), loaded from the oracle's weights, on the device"""
    import multimodal_diffusion_amd as A
    core = A.MMDiT(d_model=512, n_layers=n_layers, n_heads=8, mlp_ratio=4.0).eval()
    core.load_state_dict(ws["core"], strict=True)
    head = A.MultiModalNoiseHead({"video": 512, "audio": 512}, {"video": 256, "audio": 32}, hidden_dim=512).eval()
    head.load_state_dict(ws["head"], strict=True)
    av, aa = A.LinearAdapter(256, 256), A.LinearAdapter(32, 256)
    av.load_state_dict(ws["adapt_v"], strict=True)
    aa.load_state_dict(ws["adapt_a"], strict=True)
    return tuple(m.to(dev) for m in (core, head, av, aa))


# module scope, not session: a file that sets core.matmul or updates a parameter in place must not reach the next file
@pytest.fixture(scope="module")
def model(dev):
    """(ws, modules) of the 2-layer model"""
    ws = R.synth_weights(seed=0, n_layers=2)
    return ws, modules(dev, ws, 2)


@pytest.fixture(scope="module")
def full(dev):
    """(ws, modules) of the 8-layer model"""
    ws = R.synth_weights(seed=0)
    return ws, modules(dev, ws, 8)


def engine(mods, target, shape, n_prompt, *, guidance, alpha_bar=ABAR, tstep_dim=256, **kw):
    import multimodal_diffusion_amd as A
    core, head, av, aa = mods
    return A.DenoiseEngine(adapt_v=av, adapt_a=aa, core=core, head=head, tstep_dim=tstep_dim, target=target, latent_shape=shape,
                           prompt_tokens=n_prompt, alpha_bar=alpha_bar, guidance=guidance, **kw)


@contextmanager
def matmul_f32(mods):
    """the fp32 kernel family whatever the batch (the "auto" rule switches at 2,048 / 6,144 rows), so that batch sizes can be
    compared; the modules' own setting is back afterwards"""
    core, head = mods[0], mods[1]
    prev = core.matmul, head.matmul
    core.matmul = head.matmul = "f32"
    try:
        yield
    finally:
        core.matmul, head.matmul = prev


# ------------------------------------------------------------------------------------------------- small inputs
def ts(v, dev):
    """timesteps: a long tensor on the device (not `t`: the tests keep that name for a timestep)"""
    return torch.tensor(v, dtype=torch.long, device=dev)


def soft_mask(shape, seed=3):
    """per-sample mask with exact 0 and 1 entries and fractional ones"""
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(shape, generator=g)
    m[m < 0.35] = 0.0
    m[m > 0.7] = 1.0
    assert (m == 0).any() and (m == 1).any() and ((m > 0) & (m < 1)).any()
    return m


def _drawn(dev, seed, shape, prompt_shape, n_prompt, known):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(shape, generator=g)
    zp = torch.randn(prompt_shape, generator=g)
    if not known:
        return z.to(dev), zp.to(dev), n_prompt
    return z.to(dev), zp.to(dev), n_prompt, torch.randn(shape, generator=g).to(dev)


def video_case(dev, B=2, W=32, seed=0, known=False):
    """(z, audio prompt, 10[, known]): a video latent [B, 8, 4, 16, W] and an audio prompt of 10 tokens (chunk 4, stride 4)"""
    return _drawn(dev, seed, (B, 8, 4, 16, W), (B, 8, 40), 10, known)


def audio_case(dev, B=2, L=40, seed=1, known=False):
    """(z, video prompt, 8[, known]): an audio latent [B, 8, L] and a video prompt of 8 tokens (tube 2 x 4 x 4)"""
    return _drawn(dev, seed, (B, 8, L), (B, 8, 4, 8, 8), 8, known)


def case(dev, target, B=2, seed=0, W=32):
    """(z, prompt, prompt tokens, known) of either target, from one generator"""
    return video_case(dev, B, W, seed, known=True) if target == "video" else audio_case(dev, B, 40, seed, known=True)


def grp(g, prefix):
    """the golden's entries named `prefix/...`, as tensors under the rest of the name"""
    return {k[len(prefix) + 1:]: torch.from_numpy(v) for k, v in g.items() if k.startswith(prefix + "/")}


# ------------------------------------------------------------------------------------------------- the reduced pipeline
def pipeline_cfg(*, clip_seconds, sampler_steps, size=(32, 32), streaming=None, sampling=None, tokenizer=None):
    """the config of the reduced pipeline: tube 2 x 4 x 4, chunk 4 / 4, 16 fps, a cosine schedule of 1000 steps; `sampling` adds to
    (or overrides) guidance 2.0 for both targets; `tokenizer` = {"video": {"tube": ...}, "audio": {"chunk": ...}} replaces the
    tokenizer sub-dicts it names"""
    cfg = {"tokenizer": {"width": 512, "video": {"tube": {"t": 2, "h": 4, "w": 4}}, "audio": {"chunk": {"length": 4, "stride": 4}}},
           "video": {"fps": 16, "size": list(size), "latent": {"channels": 8, "t_down": 4, "s_down": 8}},
           "audio": {"sr": 16000, "latent": {"channels": 8, "frames_per_clip": 150}},
           "data": {"clip_seconds": clip_seconds},
           "diffusion": {m: {"steps": 1000, "sampler_steps": sampler_steps, "schedule": "cosine", "min_beta": 1e-4, "max_beta": 0.02}
                         for m in ("video", "audio")},
           "sampling": dict({"guidance_scale": {"video": 2.0, "audio": 2.0}}, **(sampling or {}))}
    if streaming is not None:
        cfg["streaming"] = dict(streaming)
    for k in ("video", "audio"):
        if tokenizer is not None and k in tokenizer:
            cfg["tokenizer"][k] = dict(tokenizer[k])
    return cfg


def pipeline(dev, *, seed, **cfg_args):
    """(vae, codec, cfg): the VAE, then the codec, with weights from the global generator seeded with `seed`"""
    import multimodal_diffusion_amd as A
    torch.manual_seed(seed)
    vae = A.VideoVAE.from_config({"latent": {"channels": 8, "t_down": 4, "s_down": 8}}).eval().to(dev)
    codec = A.AudioCodec.from_config({"sr": 16000, "latent": {"channels": 8, "frames_per_clip": 150},
                                      "codec": {"hop_samples": 320}}).eval().to(dev)
    return vae, codec, pipeline_cfg(**cfg_args)


def components(mods, vae, codec, dev):
    """the module and device arguments of sample_one_direction / stream_generate"""
    core, head, av, aa = mods
    return dict(vid_vae=vae, aud_codec=codec, adapt_v=av, adapt_a=aa, core=core, head=head, tstep_dim=256, device=dev)


def with_sampling(cfg, **sampling):
    return dict(cfg, sampling=dict(cfg["sampling"], **sampling))


def audio_prompt(n=18000):
    wav = (0.1 * torch.randn(n, generator=torch.Generator().manual_seed(9))).numpy()      # 18000 samples: 4 windows of 0.5 s
    return dict(prompt_modality="audio", prompt_video=None, prompt_audio=wav, seed=10)


def video_prompt():
    vid = torch.randint(0, 256, (20, 32, 32, 3), generator=torch.Generator().manual_seed(11), dtype=torch.uint8).numpy()
    return dict(prompt_modality="video", prompt_video=vid, prompt_audio=None, seed=12)          # 20 frames: 4 windows of 0.5 s


class Recorder:
    """wraps a VAE / codec and keeps the latent it last decoded"""

    def __init__(self, inner):
        self.inner, self.last = inner, None

    def encode(self, x):
        return self.inner.encode(x)

    def decode(self, z):
        self.last = z.clone()
        return self.inner.decode(z)


def free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]
