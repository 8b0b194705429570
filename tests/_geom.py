"""Token geometries beyond tube 2 x 4 x 4 and chunk 4 / 4: the tables test_token_geometry_cpu.py guards and test_gpu_token_geometry.py
runs, and the fp32 mirror of the overlap-add.  No GPU, and the package is not imported here.

A video row is the latent (C, T, H, W), the tube (t, h, w), the token width D = C t h w and the form launch_unpatch (csrc/tokens.hip)
picks for it at "cfg_rows" 1: gt = min(W, 32) / w tokens make up one 128-byte latent line; the whole-line kernel runs when gt is 4 or
8, W / w is a multiple of gt and its [gt][D + 4] fp32 tile fits 64 KiB of LDS, the 16-bytes-per-lane gather form otherwise.
An audio row is the latent (Ca, F), the chunk (len, stride), the token count Na = (F - len) / stride + 1 and the frames the windows
reach, L = (Na - 1) stride + len; frames L .. F - 1 are zero padding."""
from collections import namedtuple

import numpy as np

Video = namedtuple("Video", "id lat tube D form")
Audio = namedtuple("Audio", "id lat chunk Na L")

VIDEO = [
    Video("V0", (8, 4, 16, 32), (2, 4, 4), 256, "rows8"),       # control: the geometry of every other test
    Video("V1", (8, 4, 16, 32), (1, 4, 8), 256, "rows4"),       # w = 8, t = 1
    Video("V2", (8, 4, 16, 16), (2, 2, 4), 128, "rows4"),       # h != w, D != 256
    Video("V3", (4, 6, 8, 32), (3, 2, 16), 384, "gather"),      # gt = 2, odd t
    Video("V4", (8, 4, 8, 48), (2, 4, 4), 256, "gather"),       # W / w = 12 is no multiple of gt = 8
    Video("V5", (8, 2, 8, 24), (1, 2, 4), 64, "gather"),        # W < 32 with gt = 6
    Video("V6", (16, 4, 8, 32), (2, 8, 4), 1024, "rows8"),      # 32,896 B of LDS, 8 passes of the row loop
    Video("V7", (12, 4, 8, 32), (4, 8, 8), 3072, "rows4"),      # 49,216 B of dynamic LDS (above 48 KiB), one token row per (t', h')
    Video("V8", (16, 4, 8, 32), (4, 8, 8), 4096, "gather"),     # 65,600 B would exceed the 64 KiB bound
    Video("V9", (8, 4, 8, 32), (2, 1, 16), 256, "gather"),      # h = 1, w = 16
    Video("V10", (16, 4, 8, 16), (1, 4, 4), 256, "rows4"),      # C = 16
]

AUDIO = [
    Audio("A0", (8, 40), (4, 4), 10, 40),       # control
    Audio("A1", (8, 40), (4, 2), 19, 40),       # 50 % overlap
    Audio("A2", (8, 41), (4, 3), 13, 40),       # ragged overlap (counts 1 and 2) and one zero-padded frame
    Audio("A3", (8, 12), (4, 1), 9, 12),        # up to 4 windows per frame
    Audio("A4", (8, 40), (4, 6), 7, 40),        # gaps: 2 of every 6 frames lie under no window
    Audio("A5", (4, 40), (8, 4), 9, 40),        # len 8
    Audio("A6", (2, 150), (16, 8), 17, 144),    # 6 zero-padded frames
    Audio("A7", (8, 23), (5, 2), 10, 23),       # odd len, D = 40
    Audio("A8", (16, 9), (2, 1), 8, 9),         # len 2
    Audio("A9", (8, 150), (4, 2), 74, 150),     # Ca F = 1200: two 1024-element statistics chunks
]

V = {g.id: g for g in VIDEO}
A = {g.id: g for g in AUDIO}
# the rows the kit's synthetic weights serve unchanged: token width 256 (video) / 32 (audio)
KIT_VIDEO = [g.id for g in VIDEO if g.D == 256]
KIT_AUDIO = [g.id for g in AUDIO if g.lat[0] * g.chunk[0] == 32]


def n_video_tokens(g):
    (_, T, H, W), (t, h, w) = g.lat, g.tube
    return (T // t) * (H // h) * (W // w)


def covered(g):
    """bool [F]: the frames of an audio row that lie under at least one window"""
    F, (ln, st) = g.lat[1], g.chunk
    m = np.zeros(F, dtype=bool)
    for n in range(g.Na):
        m[n * st:min(n * st + ln, F)] = True
    return m


def ola_frames_f32(tok, Ca, length, frames, stride, window=None):
    """The overlap-add mean frame by frame in fp32, in the order of avd_audio_untokens_f32 (csrc/tokens.hip, ola_gather): the windows
    over a frame in increasing order, multiply and add rounded separately, one divide by max(summed weights, 1e-8); frames under no
    window and the zero padding are 0.  tok: float32 [B, Na, Ca * length] (numpy); window: float32 [length] or None (rectangular)."""
    tok = np.asarray(tok, dtype=np.float32)
    B, Na, D = tok.shape
    assert D == Ca * length and Na == (frames - length) // stride + 1
    w = np.ones(length, np.float32) if window is None else np.asarray(window, dtype=np.float32)
    t4 = tok.reshape(B, Na, Ca, length)
    out = np.zeros((B, Ca, frames), np.float32)
    L = (Na - 1) * stride + length
    for f in range(min(L, frames)):
        acc, cnt = np.zeros((B, Ca), np.float32), np.float32(0.0)
        for n in range(Na):
            j = f - n * stride
            if 0 <= j < length:
                acc = (acc + (t4[:, n, :, j] * w[j]).astype(np.float32)).astype(np.float32)
                cnt = np.float32(cnt + w[j])
        out[:, :, f] = acc / np.maximum(cnt, np.float32(1e-8))
    return out
