"""CPU tests of the fractional prompt hop (include/avdiff_hip.h, "fractional prompt hop"): ``fifo_prompt_windows(prompt_den=,
prompt_interp=)`` against a brute-force loop in exact rationals and numpy fp32, bit for bit; the contract's edges (zeros outside the
canvas, the blend toward 0 at its end, den == 1, rem == 0 beside an inf, the tie of "nearest"); ``fifo_geometry(prompt_interp=)`` on
hand-computed cases; every new refusal, the pipeline's before an encoder is touched; and what ``avd_fifo_prompt_gather_frac_f32``
refuses before a launch."""
import inspect
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest
import torch

from _kit import pipeline_cfg
from test_stream_fifo_cpu import STREAM_ONE_SECOND, Boom, Touched, shipped_cfg

ROOT = Path(__file__).resolve().parent.parent
MODES = ("nearest", "linear")
HOPS = ((2, 3), (8, 25), (25, 8), (3, 2))


def canvases():
    g = torch.Generator().manual_seed(5)
    return {"audio": torch.randn(3, 11, generator=g), "video": torch.randn(2, 7, 4, 4, generator=g)}


def brute(canvas: torch.Tensor, qs, num: int, den: int, mode: str, Lp: int) -> torch.Tensor:
    """the contract, element by element: i0 / rem from exact rationals, the blend in numpy fp32, one operation at a time"""
    c = canvas.numpy()
    P = c.shape[1]
    out = np.zeros((len(qs), c.shape[0], Lp) + c.shape[2:], dtype=np.float32)
    zero = np.zeros(c.shape[:1] + c.shape[2:], dtype=np.float32)
    at = lambda p: c[:, p] if 0 <= p < P else zero
    for k, q in enumerate(qs):
        x = Fraction(q * num, den)
        i0 = x.numerator // x.denominator                                        # floor, also below zero
        rem = q * num - i0 * den
        assert 0 <= rem < den and Fraction(rem, den) == x - i0
        for l in range(Lp):
            if mode == "nearest":
                out[k, :, l] = at(i0 + l + (1 if 2 * rem >= den else 0))
            elif rem == 0:
                out[k, :, l] = at(i0 + l)
            else:
                a, b = at(i0 + l), at(i0 + l + 1)
                f = np.float32(rem) / np.float32(den)
                d = (b - a).astype(np.float32)
                out[k, :, l] = a + (f * d).astype(np.float32)
    return torch.from_numpy(out)


# ------------------------------------------------------------------------------------------------- fifo_prompt_windows
@pytest.mark.parametrize("kind", ["audio", "video"])
@pytest.mark.parametrize("mode", MODES)
def test_windows_equal_the_brute_force_contract(kind, mode):
    from multimodal_diffusion_amd.stream_infer import fifo_prompt_windows
    canvas = canvases()[kind]
    B, S, Lp = 3, 4, 3
    for num, den in HOPS:
        past = -(-canvas.shape[1] * den // num) + 2                              # the first slot wholly past the canvas end, and two more
        for stride in range(1, S + 1):
            for first in range(-5, past + 1):
                w = fifo_prompt_windows(canvas, 0, B, S, num, Lp, stride=stride, first=first, prompt_den=den, prompt_interp=mode)
                ref = brute(canvas, [first + k * stride for k in range(B)], num, den, mode, Lp)
                assert w.dtype == torch.float32 and torch.equal(w, ref), (num, den, stride, first)
        # the defaults of stride / first: sample k at clip slot m + k * S
        assert torch.equal(fifo_prompt_windows(canvas, 2, B, S, num, Lp, prompt_den=den, prompt_interp=mode),
                           brute(canvas, [2 + k * S for k in range(B)], num, den, mode, Lp))


@pytest.mark.parametrize("mode", MODES)
def test_zeros_outside_the_canvas_and_the_blend_toward_zero(mode):
    from multimodal_diffusion_amd.stream_infer import fifo_prompt_windows
    audio = canvases()["audio"].abs() + 1.0                                      # no zero in the canvas: a zero is padding
    P, Lp = audio.shape[1], 4
    win = lambda q, num, den: fifo_prompt_windows(audio, 0, 1, 1, num, Lp, first=q, prompt_den=den, prompt_interp=mode)[0]
    # hop 2/3: slot -5 is i0 = -4, rem = 2: rows -4 .. -1 ("linear": each blended with its right neighbour, row -1 with canvas row 0)
    w = win(-5, 2, 3)
    if mode == "nearest":                                                        # 2 * 2 >= 3: one up, rows -3 .. 0
        assert (w[:, :3] == 0).all() and torch.equal(w[:, 3], audio[:, 0])
    else:
        f = torch.tensor(2, dtype=torch.float32) / 3
        assert (w[:, :3] == 0).all() and torch.equal(w[:, 3], 0 + f * (audio[:, 0] - 0))
    assert (win(-9, 2, 3) == 0).all()                                            # i0 = -6, rem = 0: rows -6 .. -3 in both modes
    # slot 13 is i0 = 8, rem = 2: rows 8 .. 11 of 11; the last in-canvas row (10) blends toward the zero past the end
    w = win(13, 2, 3)
    if mode == "nearest":                                                        # rows 9, 10, then past the end
        assert torch.equal(w[:, :2], audio[:, 9:11]) and (w[:, 2:] == 0).all()
    else:
        a, b = audio[:, 8:11], torch.cat([audio[:, 9:11], torch.zeros(3, 1)], 1)
        assert torch.equal(w[:, :3], a + f * (b - a)) and (w[:, 3] == 0).all()
        assert (w[:, 2].abs() < audio[:, 10].abs()).all() and (w[:, 2] != 0).all()
    assert (win(-(-P * 3 // 2), 2, 3) == 0).all()                                # the first slot with i0 >= P
    assert (win(10 ** 6, 2, 3) == 0).all()


@pytest.mark.parametrize("kind", ["audio", "video"])
def test_den_1_is_the_integer_walk_bit_for_bit(kind):
    from multimodal_diffusion_amd.stream_infer import fifo_prompt_windows
    canvas = canvases()[kind]
    canvas[0, 3] = float("inf")                                                  # a blend would turn its neighbours into inf / NaN
    for hop in (1, 2):
        for first in range(-5, 9):
            for stride in (1, 3):
                ref = fifo_prompt_windows(canvas, 0, 3, 3, hop, 3, stride=stride, first=first)
                for mode in MODES:
                    w = fifo_prompt_windows(canvas, 0, 3, 3, hop, 3, stride=stride, first=first, prompt_den=1, prompt_interp=mode)
                    assert torch.equal(w, ref), (hop, first, stride, mode)
    assert torch.equal(fifo_prompt_windows(canvas, 1, 2, 2, 2, 3, prompt_den=1), fifo_prompt_windows(canvas, 1, 2, 2, 2, 3))


def test_rem_0_rows_are_the_integer_gather_beside_an_inf():
    from multimodal_diffusion_amd.stream_infer import fifo_prompt_windows
    audio = canvases()["audio"]
    audio[:, 4] = float("inf")                                                   # the right neighbour of row 3
    # hop 2/3: slots 0, 3, 6 have rem == 0 and start at rows 0, 2, 4; the window of slot 3 is rows 2 and 3
    w = fifo_prompt_windows(audio, 0, 3, 3, 2, 2, prompt_den=3, prompt_interp="linear")
    ref = fifo_prompt_windows(audio, 0, 3, 1, 2, 2)                              # slots 0, 3, 6 at hop 2/3 = slots 0, 1, 2 at hop 2
    assert torch.equal(w, ref) and torch.isfinite(w[1, :, 0]).all() and torch.isinf(w[2, :, 0]).all()
    lone = fifo_prompt_windows(audio, 0, 1, 1, 2, 2, first=3, prompt_den=3, prompt_interp="linear")[0]
    assert torch.equal(lone[:, 1], audio[:, 3])                                  # row 3 itself: b = inf is not read, 0 * inf would be NaN
    # rem != 0 does read it: slot 4 is i0 = 2, rem = 2, rows 2 and 3 blend with 3 and 4
    assert not torch.isfinite(fifo_prompt_windows(audio, 0, 1, 1, 2, 2, first=4, prompt_den=3, prompt_interp="linear")[0][:, 1]).any()


def test_nearest_ties_round_up():
    from multimodal_diffusion_amd.stream_infer import fifo_prompt_windows
    audio = canvases()["audio"]
    for q in (-3, -1, 1, 3, 5):                                                  # hop 3/2: odd slots have 2 * rem == den
        i0 = (3 * q) // 2
        assert 3 * q - 2 * i0 == 1
        w = fifo_prompt_windows(audio, 0, 1, 1, 3, 2, first=q, prompt_den=2, prompt_interp="nearest")[0]
        ref = fifo_prompt_windows(audio, 0, 1, 1, 1, 2, first=i0 + 1)[0]         # rows i0 + 1, i0 + 2
        assert torch.equal(w, ref), q
    w = fifo_prompt_windows(audio, 0, 1, 1, 8, 2, first=1, prompt_den=25, prompt_interp="nearest")[0]      # rem 8: 16 < 25 stays
    assert torch.equal(w, audio[:, 0:2])
    w = fifo_prompt_windows(audio, 0, 1, 1, 8, 2, first=2, prompt_den=25, prompt_interp="nearest")[0]      # rem 16: 32 >= 25 goes up
    assert torch.equal(w, audio[:, 1:3])


# ------------------------------------------------------------------------------------------------- geometry
def reduced_cfg(sampler_steps=12):
    """1 s windows every 0.5 s, an audio latent of 24 frames: 6 slots of 4 under a video prompt of 4 latent frames, hop 4 * 4 / 24"""
    cfg = pipeline_cfg(clip_seconds=1.0, sampler_steps=sampler_steps, streaming=STREAM_ONE_SECOND)
    cfg["audio"]["latent"]["frames_per_clip"] = 24
    return cfg


def test_geometry_returns_the_reduced_fraction():
    from multimodal_diffusion_amd.stream_infer import FifoGeometry, fifo_geometry
    cfg = shipped_cfg()
    for mode in MODES:
        g = fifo_geometry(cfg, "video", 3, 37, prompt_interp=mode)
        assert (g.S, g.slot_len, g.prompt_hop, g.prompt_den, g.B) == (37, 4, 8, 25, 1)
        assert (g.hop_t, g.L_t, g.hop_p, g.L_p, g.P, g.n_slots, g.P_p) == (50, 150, 4, 12, 250, 63, 20)
    assert fifo_geometry(cfg, "video", 3, 74, prompt_interp="linear").B == 2
    with pytest.raises(ValueError, match=r"50 steps.*37 and 74"):
        fifo_geometry(cfg, "video", 3, 50, prompt_interp="linear")
    with pytest.raises(ValueError, match=r"the prompt has 0\.32 latent positions per target slot.*whole positions"):
        fifo_geometry(cfg, "video", 3, 37)                                       # without a mode: today's refusal
    with pytest.raises(ValueError, match="prompt_interp must be None or one of"):
        fifo_geometry(cfg, "video", 3, 37, prompt_interp="cubic")
    # a whole hop stays whole under a mode; the new field is the last one and defaults to 1
    g = fifo_geometry(cfg, "audio", 3, 48, prompt_interp="nearest")
    assert (g.prompt_hop, g.prompt_den) == (25, 1) and g == fifo_geometry(cfg, "audio", 3, 48)
    assert FifoGeometry._fields[-1] == "prompt_den" and FifoGeometry._field_defaults == {"prompt_den": 1}
    assert inspect.signature(fifo_geometry).parameters["prompt_interp"].default is None
    g = fifo_geometry(reduced_cfg(), "video", 3, 12, prompt_interp="linear")
    assert (g.S, g.slot_len, g.prompt_hop, g.prompt_den, g.B, g.L_t, g.L_p) == (6, 4, 2, 3, 2, 24, 4)
    with pytest.raises(ValueError, match=r"5 steps.*S = 6"):
        fifo_geometry(reduced_cfg(), "video", 3, 5, prompt_interp="linear")
    # 1 s windows at the shipped rate of 50 audio latent frames per second: S = 12, 4 * 4 / 50 = 8 / 25 as at 3 s; the kit's own 1 s
    # config keeps 150 frames per window: 4 * 4 / 150 = 8 / 75
    cfg = pipeline_cfg(clip_seconds=1.0, sampler_steps=12, streaming=STREAM_ONE_SECOND)
    g = fifo_geometry(cfg, "video", 3, 37, prompt_interp="nearest")
    assert (g.L_t, g.S, g.prompt_hop, g.prompt_den) == (150, 37, 8, 75)
    cfg["audio"]["latent"]["frames_per_clip"] = 50
    g = fifo_geometry(cfg, "video", 3, 12, prompt_interp="nearest")
    assert (g.L_t, g.S, g.prompt_hop, g.prompt_den) == (50, 12, 8, 25)


# ------------------------------------------------------------------------------------------------- refusals
def test_refusals_of_the_python_layers():
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import functional as Fn
    from multimodal_diffusion_amd.stream_infer import fifo_prompt_windows
    audio = canvases()["audio"]
    with pytest.raises(ValueError, match="prompt_interp must be None or one of"):
        fifo_prompt_windows(audio, 0, 1, 1, 2, 2, prompt_den=3, prompt_interp="cubic")
    with pytest.raises(ValueError, match="prompt_den 3 > 1.*needs prompt_interp"):
        fifo_prompt_windows(audio, 0, 1, 1, 2, 2, prompt_den=3)
    for bad in (0, -1, 2 ** 31, True, 1.5):
        with pytest.raises(ValueError, match="prompt_den must be an int"):
            fifo_prompt_windows(audio, 0, 1, 1, 2, 2, prompt_den=bad, prompt_interp="linear")
    with pytest.raises(ValueError, match="blends in float32"):
        fifo_prompt_windows(audio.double(), 0, 1, 1, 2, 2, prompt_den=3, prompt_interp="linear")
    # fifo_denoise checks the pair before it looks at the engine's state
    eng = object.__new__(A.DenoiseEngine)
    args = (eng, torch.zeros(8, 4, 4, 4), 2, torch.tensor([999, 749, 499, 249, -1]), 3, 1)
    with pytest.raises(ValueError, match="needs prompt_interp"):
        A.fifo_denoise(*args, prompt_den=3)
    with pytest.raises(ValueError, match="prompt_interp must be None or one of"):
        A.fifo_denoise(*args, prompt_den=3, prompt_interp="cubic")
    with pytest.raises(ValueError, match="prompt_den must be an int"):
        A.fifo_denoise(*args, prompt_den=0, prompt_interp="linear")
    sig = inspect.signature(A.fifo_denoise).parameters
    assert sig["prompt_den"].default == 1 and sig["prompt_interp"].default is None
    sig = inspect.signature(A.DenoiseEngine.fifo_open).parameters
    assert sig["prompt_den"].default == 1 and sig["prompt_interp"].default is None
    # the device form refuses a CPU canvas before anything else, like its integer neighbour
    with pytest.raises(ValueError, match="contiguous float32 device tensor"):
        Fn.fifo_prompt_gather_frac(audio, None, 1, 0, 1, 2, 3, "linear", 2)
    assert Fn.PROMPT_INTERPS == MODES


def test_the_pipeline_checks_prompt_interp_before_any_encoder():
    from multimodal_diffusion_amd import stream_infer as S
    cfg = reduced_cfg()
    vid = np.zeros((40, 32, 32, 3), dtype=np.uint8)                              # 40 frames at 16 fps: 4 windows of 1.0 s every 0.5 s
    kw = dict(cfg=cfg, vid_vae=Boom(), aud_codec=Boom(), adapt_v=None, adapt_a=None, core=None, head=None, tstep_dim=256,
              device=torch.device("cpu"), prompt_modality="video", prompt_video=vid, prompt_audio=None)
    for bad in ("cubic", 1, True, ["linear"]):
        with pytest.raises(ValueError, match=r"fifo\['prompt_interp'\]"):
            S.stream_generate(sampler="fifo", fifo={"prompt_interp": bad}, **kw)
    with pytest.raises(ValueError, match=r"fifo\['prompt_interp'\]"):             # the config's own setting is refused like the argument
        S.stream_generate(sampler="fifo", **dict(kw, cfg=dict(cfg, streaming=dict(STREAM_ONE_SECOND, fifo={"prompt_interp": "cubic"}))))
    with pytest.raises(ValueError, match="whole positions"):                     # absent or None: today's refusal
        S.stream_generate(sampler="fifo", **kw)
    with pytest.raises(ValueError, match="whole positions"):
        S.stream_generate(sampler="fifo", fifo={"prompt_interp": None}, **kw)
    with pytest.raises(ValueError, match=r"5 steps.*6"):                         # a mode lets the geometry through to its next check
        S.stream_generate(sampler="fifo", fifo={"prompt_interp": "linear", "steps": 5}, **kw)
    with pytest.raises(Touched, match="encode"):                                 # and a fitting step count reaches the prompt encoder
        S.stream_generate(sampler="fifo", fifo={"prompt_interp": "linear", "steps": 12}, **kw)


# ------------------------------------------------------------------------------------------------- the C entry
P0, BIG = 4096, 1 << 30                             # non-null, 16-byte aligned stand-ins: nothing is dereferenced


def test_header_and_bindings_name_the_fractional_gather():
    from multimodal_diffusion_amd import _lib as L
    header = (ROOT / "include" / "avdiff_hip.h").read_text()
    assert set(re.findall(r"\b(avd_[a-z0-9_]+)\s*\(", header)) == set(L.SIGNATURES)
    assert "avd_fifo_prompt_gather_frac_f32" in L.SIGNATURES and hasattr(L.lib(), "avd_fifo_prompt_gather_frac_f32")
    assert "fractional prompt hop (a public contract)" in header
    assert header.index("FIFO device cursors") < header.index("fractional prompt hop (a public contract)") < header.index("---- latent guide")


def test_the_c_entry_refuses_before_any_launch():
    from multimodal_diffusion_amd import _lib as L
    lib = L.lib()

    def run(canvas=2 * BIG, cursor=P0, out=3 * BIG, B=2, first=0, stride=6, num=2, den=3, interp=1, outer=8, P=10, prompt_len=4, inner=16):
        return lib.avd_fifo_prompt_gather_frac_f32(canvas, cursor, out, B, first, stride, num, den, interp, outer, P, prompt_len, inner, None)

    for kw in (dict(num=0), dict(den=0), dict(num=-1), dict(den=-3)):
        assert run(**kw) == L.EINVAL and b"num >= 1 and den >= 1" in lib.avd_last_error(), kw
    for interp in (-1, 2, 7):
        assert run(interp=interp) == L.EINVAL and b"interp must be 0 (nearest) or 1 (linear)" in lib.avd_last_error(), interp
    n_c = 8 * 10 * 16 * 4                                                        # the canvas's bytes; out is 2 * 8 * 4 * 16 floats
    assert run(out=2 * BIG + n_c - 4) == L.EINVAL and b"overlap" in lib.avd_last_error()
    assert run(out=2 * BIG - 4) == L.EINVAL and b"overlap" in lib.avd_last_error()
    assert run(out=2 * BIG, cursor=None) == L.EINVAL and b"overlap" in lib.avd_last_error()
    # what the integer gather checks
    assert run(canvas=None) == L.EINVAL and run(out=None) == L.EINVAL and b"null pointer" in lib.avd_last_error()
    for kw in (dict(B=0), dict(stride=0), dict(outer=0), dict(P=0), dict(prompt_len=0), dict(inner=0)):
        assert run(**kw) == L.EINVAL and b"bad dims" in lib.avd_last_error(), kw
    # the ranges of the walk
    for kw in (dict(first=2 ** 31), dict(first=-2 ** 31), dict(B=2 ** 16, stride=2 ** 15), dict(prompt_len=2 ** 31)):
        assert run(**kw) == L.EINVAL and b"below 2^31" in lib.avd_last_error(), kw
    assert run(first=2 ** 31 - 1, num=2 ** 31 - 1, cursor=None) == L.EINVAL and b"64-bit range" in lib.avd_last_error()
    # off a cursor the largest slot is the cursor's clamp, the first value from which every window is past P: it counts as well
    assert run(P=2 ** 50, den=2 ** 20, num=2 ** 31 - 1) == L.EINVAL and b"64-bit range" in lib.avd_last_error()
