"""CPU-only checks of the seeded DDIM noise stream (no GPU, no kernel launches): the numpy Philox4x32-10 reference reproduces the
Random123 known-answer vectors, its Box-Muller stays finite at both ends of u, the header declares the two seeded entry points and
_lib binds them, and avd_gaussian_noise_f32 refuses bad arguments before any HIP call."""
import ctypes as C
import re

import numpy as np
import pytest

from _noise_ref import box_muller, normals, philox4x32_10
from conftest import ROOT


def _words(s):
    return [int(w, 16) for w in s.split()]


@pytest.mark.parametrize("ctr,key,expect", [
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, expect):
    out = philox4x32_10([np.uint32(w) for w in _words(ctr)], [np.uint32(w) for w in _words(key)])
    assert [int(x) for x in out] == _words(expect)


def test_box_muller_finite_at_both_ends():
    # xa >> 8 = 0 -> u = 2^-24 (the largest radius); xa >> 8 = 2^24 - 1 -> u = 1 (radius 0)
    xa = np.array([0x000000FF, 0xFFFFFFFF], dtype=np.uint32)
    xb = np.array([0x12345678, 0x00000000], dtype=np.uint32)
    ne, no = box_muller(xa, xb)
    assert np.isfinite(ne).all() and np.isfinite(no).all()
    r_max = np.sqrt(-2.0 * np.log(2.0 ** -24))
    assert abs(np.hypot(ne[0], no[0]) - r_max) < 1e-12
    assert ne[1] == 0.0 and no[1] == 0.0


def test_reference_stream_layout():
    """Element e of a row takes value e & 3 of the Philox call at counter e >> 2; rows differ by sample and timestep."""
    a = normals(7, 3, [5, 5], 10)
    assert a.shape == (2, 10)
    b = normals(7, 4, [5], 10)
    assert np.array_equal(a[1], b[0])                         # the row of sample 4 does not depend on the batch around it
    c = normals(7, 3, [5, 6], 10)
    assert np.array_equal(a[0], c[0]) and not np.allclose(a[1], c[1])
    # e = 8, 9, 10 of sample 3 at t = 5: counter (2, 3, 5, tag), values 0, 1 (from x0, x1) and 2 (from x2, x3)
    d = normals(7, 3, [5], 11)[0]
    assert np.array_equal(d[:10], a[0])
    x = philox4x32_10((np.uint32(2), np.uint32(3), np.uint32(5), np.uint32(0x44444D31)), (np.uint32(7), np.uint32(0)))
    n0, n1 = box_muller(x[0], x[1])
    n2, _ = box_muller(x[2], x[3])
    assert (d[8], d[9], d[10]) == (n0, n1, n2)


def test_header_declares_and_lib_binds_seeded_entries():
    from multimodal_diffusion_amd import _lib as L
    header = (ROOT / "include" / "avdiff_hip.h").read_text()
    declared = set(re.findall(r"\b(avd_[a-z0-9_]+)\s*\(", header))
    for name in ("avd_denoise_step_seeded_f32", "avd_gaussian_noise_f32"):
        assert name in declared and name in L.SIGNATURES
        assert hasattr(L.lib(), name)
    assert "avd_noise_key" in header and "0x44444D31" in header
    assert [f[0] for f in L.NoiseKey._fields_] == ["seed", "sample_offset"] and C.sizeof(L.NoiseKey) == 16


def test_gaussian_noise_argument_errors_without_gpu():
    from multimodal_diffusion_amd import _lib as L
    lib = L.lib()
    key = L.NoiseKey(1, 0)
    assert lib.avd_gaussian_noise_f32(None, 16, 16, 4, 100, None) == L.EINVAL
    assert b"null" in lib.avd_last_error()
    assert lib.avd_gaussian_noise_f32(C.byref(key), 16, 16, 0, 100, None) == L.EINVAL
    assert b"B must be > 0" in lib.avd_last_error()
    assert lib.avd_gaussian_noise_f32(C.byref(key), None, 16, 4, 100, None) == L.EINVAL
    assert b"null pointer" in lib.avd_last_error()
    assert lib.avd_gaussian_noise_f32(C.byref(key), 16, 16, 4, 1 << 34, None) == L.EINVAL
    assert b"per_sample" in lib.avd_last_error()
    assert lib.avd_gaussian_noise_f32(C.byref(key), 16, 16, 4, 0, None) == L.EINVAL
    for off in ((1 << 32) - 3, -1):
        assert lib.avd_gaussian_noise_f32(C.byref(L.NoiseKey(1, off)), 16, 16, 4, 100, None) == L.EINVAL
        assert b"sample_offset" in lib.avd_last_error()
    assert lib.avd_denoise_step_seeded_f32(None, C.byref(key), 16, 16, 16, 16, 16, 16, 1 << 20, None) == L.EINVAL
    assert lib.avd_denoise_step_seeded_f32(C.byref(L.StepDesc()), None, 16, 16, 16, 16, 16, 16, 1 << 20, None) == L.EINVAL
    assert b"noise key" in lib.avd_last_error()


def test_python_key_validation_without_gpu():
    from multimodal_diffusion_amd import functional as Fn
    k = Fn.noise_key(2 ** 64 - 1, 5)
    assert k.seed == 2 ** 64 - 1 and k.sample_offset == 5
    for bad in (-1, 2 ** 64, 1.5, True):
        with pytest.raises(ValueError):
            Fn.noise_key(bad)
    with pytest.raises(ValueError):
        Fn.noise_key(1, -1)
