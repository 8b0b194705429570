"""CPU tests of the clip-keyed slot noise (include/avdiff_hip.h, "clip-keyed slot noise"): the numpy mirror's keying, the independence
of its domain tag from the stream a FIFO slot is initialised from, the keys a FIFO queue draws under ``fifo_slot_keying``, and the
bindings and argument checks of the new entries."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import _noise_ref as NR
import _slot_noise_ref as SN

ROOT = Path(__file__).resolve().parent.parent
NEW = ("avd_slot_noise_f32", "avd_cfg_unpatch_ddim_slots_seeded_f32", "avd_cfg_untoken_ddim_audio_slots_seeded_f32",
       "avd_denoise_step_slots_seeded_f32")
SEED = 1234


# ------------------------------------------------------------------------------------------------- the mirror's keying
def test_a_clip_position_has_one_value_however_it_is_named():
    """p = (first + b * stride) * slot_len + l: every decomposition that names a position gives its normals"""
    per, t = 24, 749
    want = SN.position_normals(SEED, range(40), [t] * 40, per)                       # positions 0 .. 39, as rows
    for first, stride, slot_len, B, S in ((0, 2, 4, 5, 2), (3, 1, 2, 4, 3), (-2, 4, 2, 3, 4), (0, 5, 8, 1, 5), (1, 3, 1, 6, 3)):
        tn = np.full((B, S), t)
        got = SN.normals(SEED, tn, (B, 6, S * slot_len, 4), slot_len, first=first, stride=stride)
        for b in range(B):
            for l in range(S * slot_len):
                p = (first + b * stride) * slot_len + l
                if 0 <= p < 40:
                    assert np.array_equal(got[b, :, l].reshape(-1), want[p]), (first, stride, slot_len, b, l)
    # a cursor adds to first, and a negative one reads as 0
    tn = np.full((2, 2), t)
    base = SN.normals(SEED, tn, (2, 6, 4, 4), 2, first=5)
    assert np.array_equal(SN.normals(SEED, tn, (2, 6, 4, 4), 2, first=-2, cursor=7), base)
    assert np.array_equal(SN.normals(SEED, tn, (2, 6, 4, 4), 2, first=5, cursor=-3), base)


def test_negative_first_wraps_mod_2_32():
    tn = np.full((1, 2), 999)
    neg = SN.normals(SEED, tn, (1, 3, 4, 4), 2, first=-1)                           # clip slots -1, 0: positions -2, -1, 0, 1
    want = SN.position_normals(SEED, [2 ** 32 - 2, 2 ** 32 - 1, 0, 1], [999] * 4, 12)
    assert np.array_equal(neg[0].transpose(1, 0, 2).reshape(4, 12), want)
    assert SN.clip_position(-3, 1, 2, 2, 1) == 2 ** 32 - 1 and SN.clip_position(2 ** 31, 0, 1, 2, 0) == 0


def test_timestep_comes_from_the_slot_and_the_tail_follows_the_last_slot():
    tn = np.array([[999, 749, 499]])
    got = SN.normals(SEED, tn, (1, 2, 8, 1), 2)                                     # 3 slots of 2 and a tail of 2
    for l, t in enumerate([999, 999, 749, 749, 499, 499, 499, 499]):
        assert np.array_equal(got[0, :, l, 0], SN.position_normals(SEED, [l], [t], 2)[0]), l


def test_the_slot_tag_is_independent_of_the_initialising_stream():
    """a FIFO slot starts as the old tag's normals at its positions and t = s_0, and its first step has t_now = s_0: the step's draw
    must not be that stream.  32 positions x 2048 elements: |corr| < 5 / sqrt(65536), and no element in common"""
    t = [999] * 32
    new = SN.position_normals(SEED, range(32), t, 2048)
    old = NR.normals(SEED, 0, t, 2048)
    assert new.shape == old.shape == (32, 2048)
    corr = float(np.corrcoef(new.reshape(-1), old.reshape(-1))[0, 1])
    print(f"slot tag vs DDIM tag: corr {corr:+.4f}, mean {new.mean():+.4f}, var {new.var():.4f}")
    assert abs(corr) < 5 / np.sqrt(65536)
    assert not (new == old).any()
    assert abs(new.mean()) < 5 / np.sqrt(65536) and abs(new.var() - 1) < 0.03       # var of a sample variance: 2 / N, 5 sigma = 0.028


# ------------------------------------------------------------------------------------------------- the keys a queue draws
def _walk(sched, S, ctx, n_slots):
    """{(clip slot, t_now): draws} over the ramp and ``n_slots`` steady iterations of the plain (ctx = 0) or the lookahead queue, keyed
    as the drivers key their step_slots calls"""
    from multimodal_diffusion_amd import schedule_utils as su
    off, stride = su.fifo_slot_keying(S, ctx)
    if ctx:
        rn, rp, sn, sp = su.fifo_lookahead_plan(sched, S, ctx)
    else:
        rn, rp, sn, sp = su.fifo_plan(sched, S)
        sn, sp = sn[None], sp[None]
    drawn = {}

    def step(tn, tp, m):
        for k in range(tn.shape[0]):
            for s in range(S):
                if int(tn[k, s]) != int(tp[k, s]):
                    key = (m + off + k * stride + s, int(tn[k, s]))
                    drawn[key] = drawn.get(key, 0) + 1

    for r in range(rn.shape[0]):
        step(rn[r], rp[r], 0)
    for m in range(n_slots):
        step(sn[min(m, ctx)], sp[min(m, ctx)], m)
    return drawn


def test_fifo_slot_keying():
    from multimodal_diffusion_amd import schedule_utils as su
    assert su.fifo_slot_keying(3) == (0, 3) and su.fifo_slot_keying(3, 1) == (-1, 2) and su.fifo_slot_keying(4, 3) == (-3, 1)
    for bad in ((0, 0), (3, 3), (3, -1), (3, True)):
        with pytest.raises(ValueError):
            su.fifo_slot_keying(*bad)


@pytest.mark.parametrize("n_slots", [1, 4, 9])
def test_every_finished_slot_draws_each_of_its_keys_once(n_slots):
    sched = torch.linspace(999, -1, 7).round().long()                                # 6 steps
    s = sched.tolist()
    walks = [_walk(sched, 3, ctx, n_slots) for ctx in (0, 1, 2)]
    for drawn in walks:
        assert all(v == 1 for v in drawn.values())                                   # no key is drawn twice
        for c in range(n_slots):
            assert {k for k in drawn if k[0] == c} == {(c, s[i]) for i in range(6)}, c
        assert min(k[0] for k in drawn) == 0                                         # the context slots before the clip draw nothing
    assert walks[0] == walks[1] == walks[2]                                          # the plain and the lookahead queues: one key set


# ------------------------------------------------------------------------------------------------- bindings
def test_slot_key_entries_declared_exported_and_bound():
    from multimodal_diffusion_amd import _lib as L
    from multimodal_diffusion_amd import functional as Fn
    import multimodal_diffusion_amd as A
    import inspect
    header = (ROOT / "include" / "avdiff_hip.h").read_text()
    declared = set(re.findall(r"\b(avd_[a-z0-9_]+)\s*\(", header))
    lib = L.lib()
    for name in NEW:
        assert name in declared and name in L.SIGNATURES and hasattr(lib, name), name
    assert lib.avd_abi_version() == L.ABI_VERSION == 7
    assert "clip-keyed slot noise" in header and "0x534C4F54" in header and "avd_slot_key" in header
    # the struct's layout: uint64, int64, int32 (+ pad), pointer
    assert C.sizeof(L.SlotKey) == 32 and L.SlotKey.first.offset == 8 and L.SlotKey.stride.offset == 16 and L.SlotKey.cursor.offset == 24
    for name in ("slot_noise", "slot_key", "dpmpp_2m_sde_step_slots"):
        assert callable(getattr(Fn, name)), name
    assert {"eta", "noise"} <= set(inspect.signature(Fn.ddim_step_slots).parameters)
    assert {"clip_first", "clip_stride", "clip_cursor"} <= set(inspect.signature(A.DenoiseEngine.step_slots).parameters)


def test_slot_key_checks_of_the_python_side():
    from multimodal_diffusion_amd import functional as Fn
    k = Fn.slot_key(2 ** 64 - 1, -(2 ** 32 - 1), 2 ** 31 - 1)
    assert (k.seed, k.first, k.stride, k.cursor) == (2 ** 64 - 1, -(2 ** 32 - 1), 2 ** 31 - 1, None)
    for bad in (dict(seed=-1), dict(seed=2 ** 64), dict(first=2 ** 32), dict(first=-2 ** 32), dict(first=1.0), dict(first=True),
                dict(stride=0), dict(stride=2 ** 31), dict(stride=2.0), dict(cursor=torch.zeros(1, dtype=torch.int32)),
                dict(cursor=3)):
        with pytest.raises(ValueError):
            Fn.slot_key(**dict(dict(seed=1, first=0, stride=1), **bad))


def test_seeded_slot_entries_refuse_before_any_launch():
    """argument checks run before any HIP call, so a CPU-only machine sees them"""
    from multimodal_diffusion_amd import _lib as L
    lib = L.lib()
    p, big = 4096, 1 << 30                             # non-null, 16-byte aligned stand-ins: nothing is dereferenced

    def noise(key, B=2, outer=8, L_=4, slots=2, slot_len=2, inner=256):
        return lib.avd_slot_noise_f32(None if key is None else C.byref(key), p, 2 * big, B, outer, L_, slots, slot_len, inner, None)

    good = L.SlotKey(7, 0, 2, None)
    assert noise(None) == L.EINVAL and b"null slot key" in lib.avd_last_error()
    assert noise(L.SlotKey(7, 0, 0, None)) == L.EINVAL and b"stride" in lib.avd_last_error()
    assert noise(L.SlotKey(7, 0, -1, None)) == L.EINVAL
    assert noise(L.SlotKey(7, 2 ** 32, 2, None)) == L.EINVAL and b"first" in lib.avd_last_error()
    assert noise(L.SlotKey(7, -2 ** 32, 2, None)) == L.EINVAL
    assert noise(good, outer=2 ** 20, inner=2 ** 14) == L.EINVAL and b"2^34" in lib.avd_last_error()
    assert noise(good, slots=3) == L.EINVAL and b"slots 3" in lib.avd_last_error()          # 3 slots of 2 do not fit L = 4
    assert noise(good, slot_len=0) == L.EINVAL

    def video(key, eta, slots=2, t_last=None, hist=None, z_out=2 * big):
        return lib.avd_cfg_unpatch_ddim_slots_seeded_f32(p, p, t_last, p, p, p, 1000, 2.0, eta, None if key is None else C.byref(key),
                                                         slots, hist, z_out, 2, 8, 4, 16, 32, 2, 4, 4, None)

    assert video(None, 0.5) == L.EINVAL and b"null slot key" in lib.avd_last_error()
    assert video(None, 0.0) == L.EINVAL                                                     # the key is required, read or not
    assert video(L.SlotKey(7, 0, 0, None), 0.5) == L.EINVAL and b"stride" in lib.avd_last_error()
    assert video(L.SlotKey(7, 2 ** 32, 1, None), 0.5) == L.EINVAL and b"first" in lib.avd_last_error()
    assert video(good, 0.5, slots=3) == L.EINVAL and b"slots 3" in lib.avd_last_error()
    assert video(good, -0.5) == L.EINVAL
    assert video(good, 0.5, t_last=p) == L.EINVAL and b"go together" in lib.avd_last_error()
    assert video(good, 0.5, t_last=p, hist=2 * big + 64) == L.EINVAL and b"x0_hist" in lib.avd_last_error()      # overlaps z_out
    assert video(good, 0.5, t_last=p, hist=3 * big + 4) == L.EUNSUPPORTED                  # a misaligned history

    def audio(key, eta, slots=10, stride=4):
        return lib.avd_cfg_untoken_ddim_audio_slots_seeded_f32(p, p, None, p, p, p, 1000, 2.0, eta, None if key is None else C.byref(key),
                                                               slots, None, 2 * big, 2, 8, 40, 4, stride, None)

    assert audio(None, 0.5) == L.EINVAL and b"null slot key" in lib.avd_last_error()
    assert audio(L.SlotKey(7, 0, 0, None), 0.5) == L.EINVAL and b"stride" in lib.avd_last_error()
    assert audio(good, 0.5, slots=9) == L.EINVAL and b"slots 9" in lib.avd_last_error()
    assert audio(good, 0.5, slots=19, stride=2) == L.EUNSUPPORTED and b"non-overlapping" in lib.avd_last_error()
    # the unseeded slot entries keep their eta == 0 scope: they have no eta to pass, and a slot key rides nowhere without slots
    assert lib.avd_cfg_unpatch_ddim_slots_f32(p, p, p, p, p, 1000, 2.0, 3, 2 * big, 2, 8, 4, 16, 32, 2, 4, 4, None) == L.EINVAL
