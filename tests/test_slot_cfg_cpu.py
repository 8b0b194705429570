"""CPU tests of the slot CFG control (include/avdiff_hip.h, "slot CFG control"): the bindings, the scratch size, every refusal the C
entries make before a launch, the level tables, the host-side refusals of ``set_slot_cfg`` and ``fifo_denoise``'s new arguments, and the
numpy mirror against the per-sample mirrors it is built from."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import _apg_ref as AR
import _cfg_ref as CR
import _slot_cfg_ref as SC

ROOT = Path(__file__).resolve().parent.parent
NEW = ("avd_slot_cfg_stats_bytes", "avd_cfg_unpatch_ddim_slots_cfg_f32", "avd_cfg_untoken_ddim_audio_slots_cfg_f32",
       "avd_denoise_step_slots_cfg_f32")


# ------------------------------------------------------------------------------------------------- bindings
def test_header_names_equal_the_bindings_and_abi_is_7():
    from multimodal_diffusion_amd import _lib as L
    from multimodal_diffusion_amd import schedule_utils as su
    import multimodal_diffusion_amd as A
    header = (ROOT / "include" / "avdiff_hip.h").read_text()
    declared = set(re.findall(r"\b(avd_[a-z0-9_]+)\s*\(", header))
    assert declared == set(L.SIGNATURES)
    lib = L.lib()
    for name in NEW:
        assert name in declared and hasattr(lib, name), name
    assert lib.avd_abi_version() == L.ABI_VERSION == 7
    assert "slot CFG control" in header and "avd_slot_cfg" in header
    # the struct's layout: two pointers, int32, two floats (+ pad), pointer, int64
    offs = [getattr(L.SlotCfg, f).offset for f in ("guidance_t", "rescale_t", "apg", "norm_threshold", "eta_parallel", "stats", "stats_bytes")]
    assert offs == [0, 8, 16, 20, 24, 32, 40] and C.sizeof(L.SlotCfg) == 48
    assert callable(su.level_table) and callable(su.guidance_interval_table)
    assert callable(A.DenoiseEngine.set_slot_cfg) and callable(A.DenoiseEngine.clear_slot_cfg)
    assert {"guidance", "rescale", "apg"} <= set(inspect.signature(A.DenoiseEngine.set_slot_cfg).parameters)
    assert {"guidance_by_level", "rescale_by_level", "apg"} <= set(inspect.signature(A.fifo_denoise).parameters)


def test_stats_bytes():
    from multimodal_diffusion_amd import _lib as L
    f = L.lib().avd_slot_cfg_stats_bytes
    for B, S, per in ((0, 2, 64), (2, 0, 64), (2, 2, 1), (2, 2, 0), (-1, 2, 64), (2, -3, 64), (256, 256, 64)):
        assert f(B, S, per) == -1, (B, S, per)
    assert f(255, 257, 64) > 0                                   # B * S = 65535: the last grid that fits
    # monotone in each argument, and the tail is 16 bytes per slot behind the 16-byte aligned partials (32 bytes per 1024-element chunk)
    for B, S, per in ((2, 2, 2), (2, 10, 32), (1, 3, 2304), (32, 3, 65536)):
        n = f(B, S, per)
        chunks = (per + 1023) // 1024
        assert n == ((B * S * chunks * 32 + 15) & ~15) + 16 * B * S
        assert f(B + 1, S, per) > n and f(B, S + 1, per) > n and f(B, S, per + 1024) > n and f(B, S, per + 1) >= n
    assert f(2, 2, 1024) == f(2, 2, 2) and f(2, 2, 1025) > f(2, 2, 1024)        # the partition is by 1024-element chunks


# ------------------------------------------------------------------------------------------------- refusals of the C entries
P0, BIG = 4096, 1 << 30                             # non-null, 16-byte aligned stand-ins: nothing is dereferenced


def _cfg(**kw):
    from multimodal_diffusion_amd import _lib as L
    f = dict(guidance_t=P0, rescale_t=None, apg=0, norm_threshold=0.0, eta_parallel=0.0, stats=None, stats_bytes=0)
    f.update(kw)
    return L.SlotCfg(f["guidance_t"], f["rescale_t"], f["apg"], f["norm_threshold"], f["eta_parallel"], f["stats"], f["stats_bytes"])


def test_fused_entries_refuse_before_any_launch():
    from multimodal_diffusion_amd import _lib as L
    lib = L.lib()
    B, shape, tube = 2, (8, 4, 16, 32), (2, 4, 4)
    need = lib.avd_slot_cfg_stats_bytes(B, 2, 8 * 2 * 16 * 32)
    lat = B * 8 * 4 * 16 * 32 * 4                                 # bytes of z / z_out / x0_hist; eps2 holds twice as many
    EPS, Z, OUT, HIST, ST = 1 * BIG, 2 * BIG, 3 * BIG, 4 * BIG, 5 * BIG

    def video(cfg, eta=0.0, key=None, slots=2, t_last=None, hist=None):
        return lib.avd_cfg_unpatch_ddim_slots_cfg_f32(EPS, Z, t_last, P0, P0, P0, 1000, 2.0, eta, None if key is None else C.byref(key), None,
                                                      slots, hist, OUT, B, *shape, *tube, None if cfg is None else C.byref(cfg), None)

    def bad(rc, msg, code=L.EINVAL):
        assert rc == code and msg in lib.avd_last_error(), (rc, lib.avd_last_error())

    bad(video(None), b"null slot CFG control")
    bad(video(_cfg(apg=1, rescale_t=P0, stats=ST, stats_bytes=need)), b"together with APG")
    for kw in (dict(norm_threshold=-1.0), dict(norm_threshold=float("nan")), dict(norm_threshold=float("inf"))):
        bad(video(_cfg(apg=1, stats=ST, stats_bytes=need, **kw)), b"norm_threshold")
    for eta_p in (-0.1, 1.5, float("nan")):
        bad(video(_cfg(apg=1, eta_parallel=eta_p, stats=ST, stats_bytes=need)), b"eta_parallel")
    for mode in (dict(apg=1), dict(rescale_t=P0)):
        bad(video(_cfg(**mode)), b"need the statistics scratch")
        bad(video(_cfg(stats=ST, stats_bytes=need - 1, **mode)), b"needed")
        bad(video(_cfg(stats=ST + 4, stats_bytes=need, **mode)), b"16-byte aligned", L.EUNSUPPORTED)
        for base, n in ((Z, lat), (OUT, lat), (EPS, 2 * lat)):
            bad(video(_cfg(stats=base + n - 16, stats_bytes=need, **mode)), b"must not overlap")
        bad(video(_cfg(stats=HIST + 64, stats_bytes=need, **mode), t_last=P0, hist=HIST), b"must not overlap")
    # a guidance table alone needs no scratch; everything the slot entries check still holds
    bad(video(_cfg(), slots=3), b"slots 3")
    bad(video(_cfg(), slots=0), b"slots must be > 0")
    bad(video(_cfg(), eta=0.5), b"slot key")
    bad(video(_cfg(), t_last=P0), b"go together")
    assert video(_cfg(), t_last=P0, hist=HIST + 4) == L.EUNSUPPORTED          # a misaligned history

    def audio(cfg, slots=10, stride=4, F=40):
        return lib.avd_cfg_untoken_ddim_audio_slots_cfg_f32(EPS, Z, None, P0, P0, P0, 1000, 2.0, 0.0, None, None, slots, None, OUT, 2, 8, F,
                                                            4, stride, None if cfg is None else C.byref(cfg), None)

    need_a = lib.avd_slot_cfg_stats_bytes(2, 10, 32)
    bad(audio(None), b"null slot CFG control")
    bad(audio(_cfg(apg=1, rescale_t=P0, stats=ST, stats_bytes=need_a)), b"together with APG")
    bad(audio(_cfg(rescale_t=P0, stats=ST, stats_bytes=need_a - 1)), b"needed")
    bad(audio(_cfg(rescale_t=P0, stats=ST + 8, stats_bytes=need_a)), b"16-byte aligned", L.EUNSUPPORTED)
    bad(audio(_cfg(apg=1, stats=OUT + 16, stats_bytes=need_a)), b"must not overlap")
    bad(audio(_cfg(), slots=9), b"slots 9")
    bad(audio(_cfg(), slots=19, stride=2), b"non-overlapping", L.EUNSUPPORTED)
    # the whole step refuses a null descriptor, control or key before it reads anything else
    step = lib.avd_denoise_step_slots_cfg_f32
    assert step(None, C.byref(_cfg()), None, None, None, None, P0, P0, P0, P0, 2, OUT, P0, 0, None) == L.EINVAL
    desc = L.StepDesc()
    bad(step(C.byref(desc), None, None, None, None, None, P0, P0, P0, P0, 2, OUT, P0, 0, None), b"null slot CFG control")
    desc.eta = 0.5
    bad(step(C.byref(desc), C.byref(_cfg()), None, None, None, None, P0, P0, P0, P0, 2, OUT, P0, 0, None), b"slot key")


# ------------------------------------------------------------------------------------------------- level tables
def test_level_table_takes_numbers_sequences_and_callables():
    from multimodal_diffusion_amd import schedule_utils as su
    T = 50
    a = su.level_table(3.5, T, "guidance")
    assert a.dtype == torch.float32 and a.device.type == "cpu" and tuple(a.shape) == (T,) and bool((a == 3.5).all())
    seq = [0.1 * i for i in range(T)]
    for spec in (seq, np.asarray(seq), torch.tensor(seq), torch.tensor(seq, dtype=torch.float64)):
        assert torch.equal(su.level_table(spec, T, "guidance"), torch.tensor(seq, dtype=torch.float32))
    fn = su.level_table(lambda t: 1.0 + t / T, T, "guidance")
    assert torch.equal(fn, torch.tensor([1.0 + t / T for t in range(T)], dtype=torch.float32))
    src = torch.full((T,), 2.0)
    out = su.level_table(src, T, "guidance")
    out[0] = 9.0
    assert float(src[0]) == 2.0                                                 # a copy: the caller's tensor is not aliased
    assert bool((su.level_table(torch.tensor(0.5), T, "phi", 0.0, 1.0) == 0.5).all())
    for bad in (float("nan"), float("inf"), [float("nan")] * T, lambda t: float("-inf") if t == 7 else 1.0):
        with pytest.raises(ValueError, match="finite"):
            su.level_table(bad, T, "guidance")
    for bad in (1.5, -0.1, [0.5] * (T - 1) + [1.01], lambda t: -1e-3 if t == 3 else 0.5):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            su.level_table(bad, T, "guidance_rescale", 0.0, 1.0)
    for bad in ([1.0] * (T - 1), [1.0] * (T + 1), torch.ones(2, T), []):
        with pytest.raises(ValueError, match="expected a number or 50 values"):
            su.level_table(bad, T, "guidance")
    for bad in (None, "3.5", True, lambda t: "x", lambda t: None):
        with pytest.raises(ValueError):
            su.level_table(bad, T, "guidance")
    for bad_T in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="T_train"):
            su.level_table(1.0, bad_T, "guidance")


def test_guidance_interval_table():
    from multimodal_diffusion_amd import schedule_utils as su
    tab = su.guidance_interval_table(4.0, (10, 19), 30)
    assert tab.dtype == torch.float32 and tuple(tab.shape) == (30,)
    assert bool((tab[:10] == 1.0).all()) and bool((tab[10:20] == 4.0).all()) and bool((tab[20:] == 1.0).all())      # ends inclusive
    assert bool((su.guidance_interval_table(4.0, None, 30) == 4.0).all())
    assert bool((su.guidance_interval_table(4.0, (25, 400), 30)[25:] == 4.0).all())       # an end past the table is the table's end
    for bad in ((5, 3), (-1, 4), (1.5, 4), (1, 2, 3), "ab"):
        with pytest.raises(ValueError, match="guidance_interval"):
            su.guidance_interval_table(4.0, bad, 30)
    for bad in (float("nan"), float("inf"), "4", True):
        with pytest.raises(ValueError, match="finite number"):
            su.guidance_interval_table(bad, (1, 2), 30)
    # as a level_table spec it round-trips
    assert torch.equal(su.level_table(tab, 30, "guidance"), tab)


# ------------------------------------------------------------------------------------------------- host-side refusals
def _bare_engine(shape=(2, 8, 4, 16, 16)):
    """a DenoiseEngine shell without a device: what set_slot_cfg's and fifo_denoise's checks read before they touch one"""
    import multimodal_diffusion_amd as A
    eng = object.__new__(A.DenoiseEngine)
    eng.latent_shape, eng.device, eng.target, eng.tube = shape, torch.device("cpu"), "video", (2, 4, 4)
    eng.alpha_bar, eng._clip, eng._scfg = torch.linspace(0.999, 0.01, 1000), None, None
    eng._scfg_g = eng._scfg_phi = eng._scfg_stats = None
    return eng


BAD_SLOT_CFG = [(dict(), "needs guidance, rescale or apg"),
                (dict(guidance=float("nan")), "finite"),
                (dict(guidance=[1.0] * 999), "1000 values"),
                (dict(rescale=1.5), r"\[0, 1\]"),
                (dict(rescale=lambda t: -0.5), r"\[0, 1\]"),
                (dict(apg={"norm_threshold": 1.0, "eta_parallel": 0.0, "momentum": -0.5}), "no momentum.*travel with it"),
                (dict(apg={"norm_threshold": -1.0}), "norm_threshold"),
                (dict(apg={"eta_parallel": 2.0}), "eta_parallel"),
                (dict(apg={"beta": 0.1}), "not"),
                (dict(apg=(1.0, 0.0)), "dict"),
                (dict(apg={"norm_threshold": 1.0}, rescale=0.7), "cannot be combined with guidance_rescale"),
                (dict(apg={}, rescale=lambda t: 0.3 if t == 999 else 0.0), "cannot be combined with guidance_rescale")]


@pytest.mark.parametrize("kw,match", BAD_SLOT_CFG)
def test_set_slot_cfg_checks_before_anything_changes(kw, match):
    eng = _bare_engine()
    with pytest.raises(ValueError, match=match):
        eng.set_slot_cfg(**kw)
    assert eng._scfg is None and eng._scfg_g is None and eng._scfg_phi is None and eng._scfg_stats is None


def test_a_slot_cfg_is_refused_by_step_and_run_and_cleared():
    from multimodal_diffusion_amd import _lib as L
    eng = _bare_engine()
    eng.set_slot_cfg(guidance=lambda t: 1.0 + t / 1000, rescale=0.0)            # a table alone, phi = 0 everywhere: no scratch, no device call
    assert isinstance(eng._scfg, L.SlotCfg) and eng._scfg.guidance_t and not eng._scfg.rescale_t and not eng._scfg.apg
    assert not eng._scfg.stats and eng._scfg.stats_bytes == 0 and eng._scfg_stats is None
    assert eng._scfg_g.dtype == torch.float32 and float(eng._scfg_g[500]) == np.float32(1.5)
    eng.Xp = object()
    with pytest.raises(ValueError, match=r"step takes no slot CFG control.*clear_slot_cfg"):
        eng.step(None, None, None)
    with pytest.raises(ValueError, match=r"run takes no slot CFG control"):
        eng.run(None, None)
    with pytest.raises(ValueError, match="no statistics pass"):
        eng.slot_cfg_coef()
    eng.clear_slot_cfg()
    assert eng._scfg is None


def test_fifo_denoise_checks_its_slot_cfg_arguments_first():
    """behind the DenoiseEngine type check and before every other argument (n_slots = 0 is wrong as well, and is not reached)"""
    import multimodal_diffusion_amd as A
    with pytest.raises(TypeError, match="DenoiseEngine"):
        A.fifo_denoise(object(), None, 1, None, 1, 0, guidance_by_level=float("nan"))
    eng = _bare_engine()
    args = (eng, torch.zeros(8, 40), 20, torch.tensor([999, 749, 499, 249, -1]), 0, 1)
    for kw, match in BAD_SLOT_CFG[1:]:
        kw = {{"guidance": "guidance_by_level", "rescale": "rescale_by_level"}.get(k, k): v for k, v in kw.items()}
        for extra in (dict(), dict(graph=True), dict(lookahead=1)):
            with pytest.raises(ValueError, match=match):
                A.fifo_denoise(*args, **kw, **extra)
    assert eng._scfg is None
    with pytest.raises(ValueError, match="n_slots"):                            # valid slot arguments: the next check is reached, nothing is set
        A.fifo_denoise(*args, guidance_by_level=3.0, rescale_by_level=0.0)
    assert eng._scfg is None and eng._scfg_g is None


# ------------------------------------------------------------------------------------------------- the mirror
def _tokens(B, Nt, D, seed=0):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((B, Nt, D)).astype(np.float32)
    u = (0.6 * c + 0.8 * rng.standard_normal((B, Nt, D))).astype(np.float32)
    return c, u


def test_mirror_at_S_1_is_the_per_sample_mirrors():
    B, Nt, D, T = 3, 6, 40, 1000
    c, u = _tokens(B, Nt, D)
    tn, tp = np.array([[999], [500], [17]]), np.array([[949], [450], [-1]])
    gtab, ptab = np.linspace(1.0, 6.0, T).astype(np.float32), np.linspace(0.0, 1.0, T).astype(np.float32)
    g, phi = gtab[tn[:, 0]], ptab[tn[:, 0]]
    e, coef = SC.control(c, u, tn, tp, 2.0, T, gtab, ptab)
    y = CR.combine_f32(c, u, g)
    assert np.array_equal(coef[:, 0, 0], CR.scale(c, y)) and np.array_equal(coef[:, 0, 1], g) and np.array_equal(coef[:, 0, 2], phi)
    assert np.array_equal(e, CR.cfg_rescale(c, y, phi))
    e, coef = SC.control(c, u, tn, tp, 2.0, T, gtab, None, apg=(2.5, 0.25))
    ref, _, (s, k, w) = AR.apg(c, u, g, 2.5, 0.25)
    assert np.array_equal(e, ref) and np.array_equal(coef[:, 0], np.stack([s, k, w, g], 1))
    # no table: the scalar; a table alone: the combine, s = 1, phi = 0
    e, coef = SC.control(c, u, tn, tp, 2.0, T)
    assert np.array_equal(e, CR.combine_f32(c, u, 2.0)) and np.array_equal(coef[:, 0], np.tile(np.float32([1, 2, 0, 0]), (B, 1)))
    # levels clamp into the table
    e_hi, _ = SC.control(c, u, np.array([[5000], [-7], [17]]), tp, 2.0, T, gtab)
    assert np.array_equal(e_hi, CR.combine_f32(c, u, gtab[[999, 0, 17]]))


def test_mirror_is_per_slot_holds_and_degenerate_slots():
    B, S, per_tok, D, T = 2, 3, 2, 16, 1000
    c, u = _tokens(B, S * per_tok, D, seed=1)
    c[0, 2:4], u[0, 2:4] = 0.25, 0.25                                           # slot (0, 1): cond and null one constant
    c[1, 4:6] = 0.0                                                             # slot (1, 2): S_cc == 0
    tn = np.array([[999, 749, 499], [249, 749, 999]])
    tp = np.array([[949, 699, 499], [199, 699, 949]])                           # slot (0, 2) is held
    gtab, ptab = np.linspace(1.5, 5.0, T).astype(np.float32), np.full(T, 0.7, np.float32)
    e, coef = SC.control(c, u, tn, tp, 3.0, T, gtab, ptab)
    assert coef[0, 1, 0] == 1.0                                                 # sigma_y == 0: s = 1
    assert np.array_equal(e.reshape(B, S, -1)[0, 1], np.full(per_tok * D, 0.25, np.float32))
    assert np.array_equal(coef[0, 2], SC.NEUTRAL)
    # a slot's numbers depend on the slot alone: the same slot elsewhere, among other slots, gives the same bits
    c2, u2 = _tokens(3, S * per_tok, D, seed=2)
    c2[2, 0:2], u2[2, 0:2] = c[1, 2:4], u[1, 2:4]
    tn2, tp2 = np.full((3, S), 17), np.full((3, S), -1)
    tn2[2, 0], tp2[2, 0] = tn[1, 1], tp[1, 1]
    e2, coef2 = SC.control(c2, u2, tn2, tp2, 3.0, T, gtab, ptab)
    assert np.array_equal(coef2[2, 0], coef[1, 1]) and np.array_equal(e2.reshape(3, S, -1)[2, 0], e.reshape(B, S, -1)[1, 1])
    ea, ca = SC.control(c, u, tn, tp, 3.0, T, gtab, None, apg=(1.0, 0.0))
    assert ca[1, 2, 1] == 0.0                                                   # S_cc == 0: k = 0
    assert ca[0, 1, 0] == 1.0 and ca[0, 1, 2] == ca[0, 1, 3] - np.float32(1)    # d == 0: S_dd == 0, no cap
    assert np.array_equal(ca[0, 2], SC.NEUTRAL)
    assert (ca[:, :, 0] <= 1.0).all() and (ca[1, :2, 0] < 1.0).all()            # r = 1 caps the random slots' |d|
