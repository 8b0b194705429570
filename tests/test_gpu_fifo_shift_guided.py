"""The guided FIFO queue shift on the MI355X (include/avdiff_hip.h, "Guided FIFO queue shift"): ``functional.fifo_shift(guide=)``
against ``fifo_shift`` followed by the in-place ``clip_guide_slots`` call on the tail slot, bit for bit — vector and scalar lanes,
audio, with and without history, every kind of mask, and a tail inside the canvas, across its end and past it."""
import pytest
import torch

from _kit import ABAR, dev, soft_mask  # noqa: F401  (dev is a fixture)

pytestmark = pytest.mark.gpu
SEED, GSEED, T_NOW, C_SLOT = 77, 4321, 600, 5

# (shape, slot_len): 16-byte lanes, one element per lane (inner = 90), audio (inner = 1)
LAYOUTS = {"video vec": ((2, 8, 4, 16, 16), 2), "video scalar": ((2, 8, 4, 15, 6), 2), "audio": ((2, 8, 16), 4)}


def _canvas_len(where, slot_len):
    """P for a tail slot at clip positions C_SLOT * slot_len ..: inside the canvas, across its end (P no multiple of slot_len), past it"""
    first = C_SLOT * slot_len
    return {"inside": first + 3 * slot_len, "straddle": first + 1, "past": first}[where]


@pytest.mark.parametrize("where", ["inside", "straddle", "past"])
@pytest.mark.parametrize("hist", [False, True], ids=["plain", "hist"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_guided_shift_is_the_shift_then_the_tail_pass(dev, layout, hist, where):
    from multimodal_diffusion_amd import functional as Fn
    shape, sl = LAYOUTS[layout]
    B, S = shape[0], shape[2] // sl
    P = _canvas_len(where, sl)
    assert where != "straddle" or P % sl
    g = torch.Generator().manual_seed(len(layout) + P)
    z = torch.randn(shape, generator=g).to(dev)
    h = torch.randn(shape, generator=g).to(dev) if hist else None
    cshape = shape[1:2] + (P,) + shape[3:]
    known = torch.randn(cshape, generator=g).to(dev)
    frac = soft_mask(cshape).to(dev)
    ab = ABAR.to(dev, torch.float32)
    plain = Fn.fifo_shift(z, C_SLOT, SEED, T_NOW, sl, hist=h)
    tau = torch.full((B, S), Fn.SLOT_LEAVE, dtype=torch.long, device=dev)
    tau[B - 1, S - 1] = T_NOW
    tail = (slice(B - 1, B), slice(None), slice((S - 1) * sl, S * sl))
    for name, mask, everywhere in (("none", None, False), ("frac", frac, False), ("zero", torch.zeros_like(frac), False),
                                   ("everywhere", frac, True)):
        want = plain[0].clone()
        # `first` puts clip slot C_SLOT on the tail: slot S - 1 of sample B - 1 holds clip slot first + (B - 1) * S + S - 1
        Fn.clip_guide_slots(known, tau, ab, want, mask, slot_len=sl, seed=GSEED, first=C_SLOT - B * S + 1, everywhere=everywhere, out=want)
        got = Fn.fifo_shift(z, C_SLOT, SEED, T_NOW, sl, hist=h, guide=dict(known=known, mask=mask, seed=GSEED, alpha_bar=ab,
                                                                          everywhere=everywhere))
        assert len(got) == (3 if hist else 2)
        assert torch.equal(got[0], want), (name, "z_out")
        assert torch.equal(got[1], plain[1]), (name, "popped")
        if hist:
            assert torch.equal(got[2], plain[2]), (name, "hist")
        keep = torch.ones(shape, dtype=torch.bool, device=dev)
        keep[tail] = False
        assert torch.equal(got[0][keep], plain[0][keep]), (name, "slots before the tail")
        if name == "zero" or where == "past":
            assert torch.equal(got[0], plain[0]), (name, "the plain shift's bits")
        elif name in ("none", "everywhere"):                                     # m == 1: the tail is q_p(t), not the fresh noise
            inside = min(sl, P - C_SLOT * sl)
            assert not torch.equal(got[0][tail][:, :, :inside], plain[0][tail][:, :, :inside]), name
            assert torch.equal(got[0][tail][:, :, inside:], plain[0][tail][:, :, inside:]), (name, "positions past the canvas end")


def test_engine_shift_guided_needs_a_clip_guide_and_follows_it(dev):
    """DenoiseEngine.fifo_shift(guided=) reads the engine's clip guide; checked on a shell without a model"""
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import functional as Fn
    shape, sl = LAYOUTS["video vec"]
    eng = object.__new__(A.DenoiseEngine)
    eng.latent_shape, eng.device, eng.target, eng.tube, eng._clip = shape, dev, "video", (sl, 4, 4), None
    eng.solver, eng.noise_seed, eng.alpha_bar = "ddim", None, ABAR.to(dev, torch.float32)
    g = torch.Generator().manual_seed(3)
    z = torch.randn(shape, generator=g).to(dev)
    known = torch.randn(8, 16, 16, 16, generator=g)
    with pytest.raises(ValueError, match="set_clip_guide"):
        eng.fifo_shift(z, C_SLOT, T_NOW, seed=SEED, guided="mask")
    mask = soft_mask(known.shape)
    eng.set_clip_guide(known, mask, guide_seed=GSEED)
    with pytest.raises(ValueError, match="guided must be"):
        eng.fifo_shift(z, C_SLOT, T_NOW, seed=SEED, guided=True)
    for guided, everywhere in (("mask", False), ("everywhere", True)):
        got = eng.fifo_shift(z, C_SLOT, T_NOW, seed=SEED, guided=guided)
        want = Fn.fifo_shift(z, C_SLOT, SEED, T_NOW, sl, guide=dict(known=known.to(dev), mask=mask.to(dev), seed=GSEED,
                                                                    alpha_bar=eng.alpha_bar, everywhere=everywhere))
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    plain = eng.fifo_shift(z, C_SLOT, T_NOW, seed=SEED)                          # None: the plain shift, also under a clip guide
    assert torch.equal(plain[0], Fn.fifo_shift(z, C_SLOT, SEED, T_NOW, sl)[0])
