"""CPU tests of the clip-keyed latent guide (include/avdiff_hip.h, "clip-keyed latent guide"): the bindings, every refusal the C entries
make before a launch, the numpy mirror's positions and its out-of-canvas rule, and the host-side refusals of ``set_clip_guide`` and
``fifo_denoise(init_canvas=...)``."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import _clip_guide_ref as CG
import _guide_ref as GR
import _slot_noise_ref as SN

ROOT = Path(__file__).resolve().parent.parent
NEW = ("avd_clip_guide_slots_f32", "avd_cfg_unpatch_ddim_slots_guided_f32", "avd_cfg_untoken_ddim_audio_slots_guided_f32",
       "avd_denoise_step_slots_guided_f32")
SEED = 4321


# ------------------------------------------------------------------------------------------------- bindings
def test_header_names_equal_the_bindings_and_abi_is_7():
    from multimodal_diffusion_amd import _lib as L
    from multimodal_diffusion_amd import functional as Fn
    import multimodal_diffusion_amd as A
    import inspect
    header = (ROOT / "include" / "avdiff_hip.h").read_text()
    declared = set(re.findall(r"\b(avd_[a-z0-9_]+)\s*\(", header))
    assert declared == set(L.SIGNATURES)
    lib = L.lib()
    for name in NEW:
        assert name in declared and hasattr(lib, name), name
    assert lib.avd_abi_version() == L.ABI_VERSION == 7
    assert "clip-keyed latent guide" in header and "avd_clip_guide" in header and "AVD_SLOT_LEAVE" in header
    # the struct's layout: two pointers, int64, uint64, int64, int32 (+ pad), pointer
    offs = [getattr(L.ClipGuide, f).offset for f in ("known", "mask", "P", "seed", "first", "stride", "cursor")]
    assert offs == [0, 8, 16, 24, 32, 40, 48] and C.sizeof(L.ClipGuide) == 56
    assert Fn.SLOT_LEAVE == L.SLOT_LEAVE == CG.LEAVE == -2 ** 63
    assert callable(Fn.clip_guide) and callable(Fn.clip_guide_slots)
    assert {"slot_len", "seed", "first", "stride", "cursor", "everywhere", "out"} <= set(inspect.signature(Fn.clip_guide_slots).parameters)
    assert callable(A.DenoiseEngine.set_clip_guide) and callable(A.DenoiseEngine.clear_clip_guide)
    assert {"init_canvas", "mask", "guide_seed", "guide_start"} <= set(inspect.signature(A.fifo_denoise).parameters)


# ------------------------------------------------------------------------------------------------- refusals of the C entries
P0, BIG = 4096, 1 << 30                             # non-null, 16-byte aligned stand-ins: nothing is dereferenced


def _guide(**kw):
    from multimodal_diffusion_amd import _lib as L
    f = dict(known=5 * BIG, mask=None, P=64, seed=SEED, first=0, stride=2, cursor=None)
    f.update(kw)
    return L.ClipGuide(f["known"], f["mask"], f["P"], f["seed"], f["first"], f["stride"], f["cursor"])


def test_stand_alone_pass_refuses_before_any_launch():
    from multimodal_diffusion_amd import _lib as L
    lib = L.lib()

    def run(g, z=2 * BIG, out=2 * BIG, B=2, outer=8, L_=4, slots=2, slot_len=2, inner=256, tau=P0):
        return lib.avd_clip_guide_slots_f32(None if g is None else C.byref(g), tau, P0, 1000, 0, z, out, B, outer, L_, slots, slot_len,
                                            inner, None)

    assert run(None) == L.EINVAL and b"null clip guide" in lib.avd_last_error()
    assert run(_guide(known=None)) == L.EINVAL and b"null known" in lib.avd_last_error()
    for P in (0, -1, 2 ** 32 + 1):
        assert run(_guide(P=P)) == L.EINVAL and b"[1, 2^32]" in lib.avd_last_error(), P
    assert run(_guide(), outer=2 ** 20, inner=2 ** 14) == L.EINVAL and b"2^34" in lib.avd_last_error()
    for stride in (0, -1):
        assert run(_guide(stride=stride)) == L.EINVAL and b"stride" in lib.avd_last_error()
    for first in (2 ** 32, -2 ** 32):
        assert run(_guide(first=first)) == L.EINVAL and b"first" in lib.avd_last_error()
    assert run(_guide(), slot_len=0) == L.EINVAL and b"slot_len" in lib.avd_last_error()
    assert run(_guide(), slots=3) == L.EINVAL and b"slots 3" in lib.avd_last_error()          # 3 slots of 2 do not fit L = 4
    assert run(_guide(), slots=0) == L.EINVAL
    n = 2 * 8 * 4 * 256 * 4                                                                    # the batch's bytes
    assert run(_guide(known=2 * BIG + n - 4)) == L.EINVAL and b"overlap" in lib.avd_last_error()
    assert run(_guide(mask=2 * BIG + 64)) == L.EINVAL and b"overlap" in lib.avd_last_error()
    assert run(_guide(), out=2 * BIG + 64) == L.EINVAL and b"out must be z" in lib.avd_last_error()
    assert run(_guide(), tau=None) == L.EINVAL and b"null pointer" in lib.avd_last_error()


def test_fused_guided_entries_refuse_before_any_launch():
    from multimodal_diffusion_amd import _lib as L
    lib = L.lib()
    good = L.SlotKey(7, 0, 2, None)

    def video(key, g, eta, slots=2, t_last=None, hist=None, z_out=2 * BIG):
        return lib.avd_cfg_unpatch_ddim_slots_guided_f32(P0, P0, t_last, P0, P0, P0, 1000, 2.0, eta, None if key is None else C.byref(key),
                                                         None if g is None else C.byref(g), slots, hist, z_out, 2, 8, 4, 16, 32, 2, 4, 4,
                                                         None)

    assert video(good, None, 0.5) == L.EINVAL and b"null clip guide" in lib.avd_last_error()
    assert video(None, _guide(), 0.5) == L.EINVAL and b"slot key" in lib.avd_last_error()      # the key may be null at eta == 0 only
    assert video(good, _guide(known=None), 0.0) == L.EINVAL and b"null known" in lib.avd_last_error()
    assert video(good, _guide(P=0), 0.0) == L.EINVAL and b"[1, 2^32]" in lib.avd_last_error()
    assert video(None, _guide(stride=0), 0.0) == L.EINVAL and b"stride" in lib.avd_last_error()
    assert video(None, _guide(first=2 ** 32), 0.0) == L.EINVAL and b"first" in lib.avd_last_error()
    assert video(good, _guide(), 0.5, slots=3) == L.EINVAL and b"slots 3" in lib.avd_last_error()
    assert video(good, _guide(known=2 * BIG + 64), 0.5) == L.EINVAL and b"overlap" in lib.avd_last_error()      # known over z_out
    assert video(good, _guide(mask=3 * BIG + 64), 0.5, t_last=P0, hist=3 * BIG) == L.EINVAL and b"overlap" in lib.avd_last_error()
    assert video(good, _guide(), 0.5, t_last=P0) == L.EINVAL and b"go together" in lib.avd_last_error()
    assert video(good, _guide(), 0.5, t_last=P0, hist=3 * BIG + 4) == L.EUNSUPPORTED          # a misaligned history
    # a slot key that rides along carries the guide's geometry
    for bad in (_guide(first=1), _guide(stride=3), _guide(cursor=P0)):
        assert video(good, bad, 0.5) == L.EINVAL and b"must equal the clip guide" in lib.avd_last_error()

    def audio(key, g, eta, slots=10, stride=4):
        return lib.avd_cfg_untoken_ddim_audio_slots_guided_f32(P0, P0, None, P0, P0, P0, 1000, 2.0, eta, None if key is None else C.byref(key),
                                                               None if g is None else C.byref(g), slots, None, 2 * BIG, 2, 8, 40, 4, stride,
                                                               None)

    assert audio(good, None, 0.5) == L.EINVAL and b"null clip guide" in lib.avd_last_error()
    assert audio(None, _guide(), 0.5) == L.EINVAL and b"slot key" in lib.avd_last_error()
    assert audio(good, _guide(P=2 ** 32 + 1), 0.5) == L.EINVAL and b"[1, 2^32]" in lib.avd_last_error()
    assert audio(good, _guide(), 0.5, slots=9) == L.EINVAL and b"slots 9" in lib.avd_last_error()
    assert audio(good, _guide(first=-1), 0.5) == L.EINVAL and b"must equal the clip guide" in lib.avd_last_error()
    assert audio(good, _guide(), 0.5, slots=19, stride=2) == L.EUNSUPPORTED and b"non-overlapping" in lib.avd_last_error()
    # the whole step refuses a null descriptor, guide or key before it reads anything else
    step = lib.avd_denoise_step_slots_guided_f32
    assert step(None, None, C.byref(_guide()), None, None, P0, P0, P0, P0, 2, 2 * BIG, P0, 0, None) == L.EINVAL
    desc = L.StepDesc()
    assert step(C.byref(desc), None, None, None, None, P0, P0, P0, P0, 2, 2 * BIG, P0, 0, None) == L.EINVAL
    assert b"null clip guide" in lib.avd_last_error()
    desc.eta = 0.5
    assert step(C.byref(desc), None, C.byref(_guide()), None, None, P0, P0, P0, P0, 2, 2 * BIG, P0, 0, None) == L.EINVAL
    assert b"slot key" in lib.avd_last_error()


# ------------------------------------------------------------------------------------------------- the mirror
def test_positions_are_signed_and_the_canvas_rule_has_no_wrap():
    # inside [0, 2^32) the guide's position is the slot noise's
    for first, b, stride, sl, l, cur in ((0, 1, 2, 4, 3, 0), (5, 1, 3, 2, 1, 7), (-2, 3, 4, 2, 0, -9)):
        assert CG.position(first, b, stride, sl, l, cur) == SN.clip_position(first, b, stride, sl, l, cur)
    # p = -1: the slot noise wraps it to 2^32 - 1, the guide leaves it outside every canvas
    assert CG.position(-1, 0, 2, 2, 1) == -1 and SN.clip_position(-1, 0, 2, 2, 1) == 2 ** 32 - 1
    assert not CG.in_canvas(-1, 2 ** 32) and not CG.in_canvas(-1, 8)
    # p = P is the first position past the canvas, p = P - 1 the last inside; P = 2^32 holds p = 2^32 - 1
    assert CG.position(2, 1, 2, 2, 0) == 8 and not CG.in_canvas(8, 8) and CG.in_canvas(7, 8)
    last = 2 ** 32 // 2 - 2 * 2
    assert CG.position(last, 1, 2, 2, 3) == 2 ** 32 - 1 and CG.in_canvas(2 ** 32 - 1, 2 ** 32) and not CG.in_canvas(2 ** 32, 2 ** 32)
    # a negative cursor reads as 0, a positive one adds to first
    assert CG.position(5, 1, 2, 2, 1, cursor=-3) == CG.position(5, 1, 2, 2, 1) == CG.position(-2, 1, 2, 2, 1, cursor=7)


def test_mirror_guides_in_canvas_positions_only():
    rng = np.random.default_rng(0)
    abar = np.linspace(0.999, 0.01, 1000)
    known, mask = rng.standard_normal((3, 6, 2)), rng.uniform(size=(3, 6, 2))
    mask[:, 0], mask[:, 1] = 0.0, 1.0
    z = rng.standard_normal((2, 3, 4, 2))
    tau = np.array([[500, -1], [CG.LEAVE, 250]])
    out = CG.clip_guide_slots(known, mask, tau, abar, z, SEED, 2, first=-1)      # positions: sample 0 -> -2 .. 1, sample 1 -> 2 .. 5
    assert np.array_equal(out[0, :, :2], z[0, :, :2])                            # p < 0: unguided
    assert np.array_equal(out[0, :, 2], z[0, :, 2])                              # p = 0: m == 0
    assert np.array_equal(out[0, :, 3], known[:, 1])                             # p = 1: m == 1 at tau = -1 returns x_k
    assert np.array_equal(out[1, :, :2], z[1, :, :2])                            # a left slot
    n4 = GR.known_normals(SEED, 4, 1, 6)[0].reshape(3, 2)
    q4 = np.sqrt(abar[250]) * known[:, 4] + np.sqrt(1 - abar[250]) * n4
    assert np.allclose(out[1, :, 2], (1 - mask[:, 4]) * z[1, :, 2] + mask[:, 4] * q4, rtol=0, atol=1e-15)
    every = CG.clip_guide_slots(known, mask, tau, abar, z, SEED, 2, first=-1, everywhere=True)
    assert np.array_equal(every, CG.clip_guide_slots(known, None, tau, abar, z, SEED, 2, first=-1))
    assert np.array_equal(every[0, :, 2], known[:, 0])
    # past the canvas end: nothing is guided
    assert np.array_equal(CG.clip_guide_slots(known, None, np.full((2, 2), 500), abar, z, SEED, 2, first=3), z)


# ------------------------------------------------------------------------------------------------- host-side refusals
def _bare_engine(shape=(2, 8, 4, 16, 16)):
    """a DenoiseEngine shell without a device: what set_clip_guide's and fifo_denoise's checks read before they touch one"""
    import multimodal_diffusion_amd as A
    eng = object.__new__(A.DenoiseEngine)
    eng.latent_shape, eng.device, eng.target, eng.tube, eng._clip = shape, torch.device("cpu"), "video", (2, 4, 4), None
    return eng


def test_set_clip_guide_checks_and_the_refusals_it_causes():
    from multimodal_diffusion_amd.sampler import canvas_frame_mask
    eng = _bare_engine()
    known = torch.randn(8, 10, 16, 16)
    for bad, match in ((torch.randn(8, 10, 16, 8), "known canvas shape"), (torch.randn(2, 8, 4, 16, 16), "known canvas shape"),
                       (torch.randn(8, 0, 16, 16), "known canvas shape")):
        with pytest.raises(ValueError, match=match):
            eng.set_clip_guide(bad)
    with pytest.raises(ValueError, match="broadcast"):
        eng.set_clip_guide(known, torch.ones(8, 9, 16, 16))
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        eng.set_clip_guide(known, torch.full((8, 10, 16, 16), 1.5))
    with pytest.raises(ValueError, match="seed"):
        eng.set_clip_guide(known, guide_seed=-1)
    assert eng._clip is None                                                     # everything is checked before anything changes
    eng.set_clip_guide(known, canvas_frame_mask(known.shape, 2, 5), guide_seed=9)
    assert torch.equal(eng._clip[0], known) and eng._clip[0] is not known and eng._clip[2] == 9
    assert float(eng._clip[1].sum()) == 8 * 3 * 16 * 16
    eng.Xp = object()
    with pytest.raises(ValueError, match=r"step takes no clip guide.*set_known"):
        eng.step(None, None, None)
    with pytest.raises(ValueError, match=r"run takes no clip guide"):
        eng.run(None, None)
    with pytest.raises(ValueError, match=r"fifo_open takes no clip guide.*eagerly"):
        eng.fifo_open(None, 1, 1, None, 1, 0)
    with pytest.raises(ValueError, match=r"fifo_lookahead takes no clip guide"):
        eng.fifo_lookahead(None, 1, 1)
    eng.eta, eng.noise_seed, eng.solver = 0.0, None, "ddim"
    with pytest.raises(ValueError, match=r"clip guide needs clip_first, at any eta"):
        eng.step_slots(None, None, None)
    eng.clear_clip_guide()
    assert eng._clip is None


def test_fifo_denoise_refuses_the_guide_outside_the_plain_eager_queue():
    import multimodal_diffusion_amd as A
    eng = _bare_engine()
    known = torch.randn(8, 10, 16, 16)
    args = (eng, torch.zeros(8, 40), 20, torch.tensor([999, 749, 499, 249, -1]), 3, 1)
    with pytest.raises(ValueError, match="graph=True is refused"):
        A.fifo_denoise(*args, graph=True, init_canvas=known)
    with pytest.raises(ValueError, match="lookahead > 0 is refused"):
        A.fifo_denoise(*args, lookahead=1, init_canvas=known)
    with pytest.raises(ValueError, match="guide_start"):
        A.fifo_denoise(*args, init_canvas=known, guide_start="known")
    with pytest.raises(ValueError, match="pass init_canvas"):
        A.fifo_denoise(*args, mask=torch.ones(8, 10, 16, 16))
    with pytest.raises(ValueError, match="pass init_canvas"):
        A.fifo_denoise(*args, guide_start="init")
    with pytest.raises(ValueError, match="seed"):
        A.fifo_denoise(*args, init_canvas=known, guide_seed=2 ** 64)
    assert eng._clip is None
