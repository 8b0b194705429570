"""The token-geometry tables of _geom.py and the oracle they are run against (no GPU): the launch form of every video row recomputed
from the dispatch rule, the tube round trip, the audio token counts, exact zeros where no window reaches, and the fp32 overlap-add of
the oracle against its fp64 self and, bit for bit, against the per-frame fp32 loop that the kernels implement."""
import numpy as np
import pytest
import torch

import _geom as G
from oracle import ref_cpu as R


def _form(lat, tube):
    """launch_unpatch's choice at "cfg_rows" 1 (csrc/tokens.hip)"""
    (C, _, _, W), (t, h, w) = lat, tube
    D = C * t * h * w
    gt = min(W, 32) // w
    rows = gt in (4, 8) and (W // w) % gt == 0 and D % 4 == 0 and gt * (D + 4) * 4 <= 64 * 1024
    return f"rows{gt}" if rows else "gather"


def test_tables_are_well_formed():
    assert [g.id for g in G.VIDEO] == [f"V{i}" for i in range(11)] and [g.id for g in G.AUDIO] == [f"A{i}" for i in range(10)]
    assert G.KIT_VIDEO == ["V0", "V1", "V4", "V9", "V10"]
    assert G.KIT_AUDIO == ["A0", "A1", "A2", "A3", "A4", "A5", "A6", "A8", "A9"]
    # every form of the dispatch is in the table, and so are the bounds next to which it changes
    assert {g.form for g in G.VIDEO} == {"rows8", "rows4", "gather"}
    lds = {g.id: (min(g.lat[3], 32) // g.tube[2]) * (g.D + 4) * 4 for g in G.VIDEO}
    assert lds["V6"] == 32896 and lds["V7"] == 49216 > 48 * 1024 and lds["V8"] == 65600 > 64 * 1024
    for g in G.VIDEO + G.AUDIO:
        assert int(np.prod(g.lat)) <= 16 * 1024               # a few seconds per GPU test at most


@pytest.mark.parametrize("g", G.VIDEO, ids=[g.id for g in G.VIDEO])
def test_video_row(g):
    (C, T, H, W), (t, h, w) = g.lat, g.tube
    assert T % t == 0 and H % h == 0 and W % w == 0 and w % 4 == 0 and W % 4 == 0
    assert g.D == C * t * h * w
    assert g.form == _form(g.lat, g.tube)
    z = torch.randn(2, *g.lat, generator=torch.Generator().manual_seed(1))
    tok = R.tube_patch(z, t, h, w)
    assert tuple(tok.shape) == (2, G.n_video_tokens(g), g.D)
    assert torch.equal(R.tube_unpatch(tok, C, T, H, W, t, h, w), z)
    # token n = (t', h', w') row-major, feature k = (c, dt, dy, dx) row-major: one entry spelled out
    n, k = G.n_video_tokens(g) - 1, g.D - 1
    assert tok[1, n, k] == z[1, C - 1, T - 1, H - 1, W - 1] and tok[1, 0, 0] == z[1, 0, 0, 0, 0]
    if W // w > 1:
        assert tok[0, 1, 0] == z[0, 0, 0, 0, w]


@pytest.mark.parametrize("g", G.AUDIO, ids=[g.id for g in G.AUDIO])
def test_audio_row(g):
    (Ca, F), (ln, st) = g.lat, g.chunk
    assert F >= ln and g.Na == (F - ln) // st + 1 and g.L == (g.Na - 1) * st + ln and g.L <= F
    z = torch.randn(2, Ca, F, generator=torch.Generator().manual_seed(2))
    tok = R.audio_tokens(z, ln, st)
    assert tuple(tok.shape) == (2, g.Na, Ca * ln)
    cov = torch.from_numpy(G.covered(g))
    assert int(cov.sum()) == {"A2": 40, "A4": 28, "A6": 144}.get(g.id, F)
    for hann in (False, True):
        back = R.audio_untokens(tok, Ca, ln, F, st, hann=hann)
        assert tuple(back.shape) == (2, Ca, F)
        assert bool((back[..., ~cov] == 0).all())              # no window, or the zero padding: exact zeros
        if not hann:                                           # the mean of equal values is the value
            assert torch.allclose(back[..., cov], z[..., cov], rtol=0, atol=1e-6)


@pytest.mark.parametrize("hann", [False, True], ids=["rect", "hann"])
@pytest.mark.parametrize("g", G.AUDIO, ids=[g.id for g in G.AUDIO])
def test_overlap_add_reference_in_fp32(g, hann):
    (Ca, F), (ln, st) = g.lat, g.chunk
    tok = torch.randn(3, g.Na, Ca * ln, generator=torch.Generator().manual_seed(3))
    f32 = R.audio_untokens(tok, Ca, ln, F, st, hann=hann)
    f64 = R.audio_untokens(tok.double(), Ca, ln, F, st, hann=hann)
    assert f32.dtype == torch.float32
    assert float((f32.double() - f64).abs().max()) < 1e-6
    win = torch.hann_window(ln).numpy() if hann else None
    assert np.array_equal(f32.numpy(), G.ola_frames_f32(tok.numpy(), Ca, ln, F, st, win))
