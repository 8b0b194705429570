"""CPU-only checks of the null-half dedup switch (include/avdiff_hip.h, avd_cfg_dedup_set; no GPU, no kernel launches): the switch
returns the previous value and round-trips, the step's workspace plan does not depend on it, the header declares it, _lib binds it
and the pinned ABI stays."""
import ctypes as C
import re

from conftest import ROOT


def test_header_declares_lib_binds_and_abi_stays():
    from multimodal_diffusion_amd import _lib as L
    header = (ROOT / "include" / "avdiff_hip.h").read_text()
    declared = set(re.findall(r"\b(avd_[a-z0-9_]+)\s*\(", header))
    assert "avd_cfg_dedup_set" in declared and "avd_cfg_dedup_set" in L.SIGNATURES and hasattr(L.lib(), "avd_cfg_dedup_set")
    assert set(L.SIGNATURES) == declared
    assert L.ABI_VERSION == 7 and L.lib().avd_abi_version() == 7
    # a switch of its own, not a tune key: the header's tune-key paragraph does not name it and avd_tune_set does not know it
    block = header[header.index("Measurement / test hooks"):header.index("int         avd_tune_set")]
    assert "dedup" not in block
    assert L.lib().avd_tune_set(b"cfg_dedup", 1) == L.EINVAL


def test_switch_returns_the_previous_value():
    from multimodal_diffusion_amd import _lib as L
    f = L.lib().avd_cfg_dedup_set
    first = f(0)
    try:
        assert first in (0, 1)
        assert f(1) == 0 and f(1) == 1 and f(0) == 1 and f(0) == 0
        assert f(7) == 0 and f(0) == 1          # any non-zero value is "on", stored as 1
    finally:
        f(first)
    assert f(first) == first


def _tables(L, n_layers=3, d=512, hidden=2048, fake=1 << 20):
    """core / head weight tables whose pointers are small integers nobody dereferences: sizing reads which are set, never what"""
    blocks = (L.BlockWeights * n_layers)()
    for b in blocks:
        for name, _ in L.BlockWeights._fields_:
            if name != "f16x2_scale":
                setattr(b, name, fake)
    core = L.CoreWeights(d, n_layers, 8, hidden, 1e-6, blocks, fake, 0, None, 6, 0)
    head = L.HeadWeights()
    head.d_in, head.hidden, head.d_out, head.n_shared = d, 512, 256, 0
    head.input_proj_weight = head.input_proj_bias = head.out_proj_weight = head.out_proj_bias = fake
    head.split_terms, head.input_proj_weight3, head.out_proj_weight3 = 6, fake, fake
    return blocks, core, head


def test_workspace_plan_does_not_depend_on_the_switch():
    from multimodal_diffusion_amd import _lib as L
    lib = L.lib()
    blocks, core, head = _tables(L)
    sizes = {}
    for B, W, Np in ((2, 32, 10), (3, 32, 70), (32, 64, 37)):
        s = L.StepDesc()
        e = s.embed
        e.target_kind, e.target_first, e.B, e.d, e.tdim = 0, 1, B, 512, 256
        e.C, e.T, e.H, e.W, e.p0, e.p1, e.p2 = 8, 4, 16, W, 2, 4, 4
        e.Nt, e.Np = 2 * 4 * (W // 4), Np
        s.core, s.head = C.pointer(core), C.pointer(head)
        s.T_train, s.guidance = 1000, 3.5
        prev = lib.avd_cfg_dedup_set(0)
        try:
            off = lib.avd_step_workspace_bytes(C.byref(s))
            lib.avd_cfg_dedup_set(1)
            on = lib.avd_step_workspace_bytes(C.byref(s))
        finally:
            lib.avd_cfg_dedup_set(prev)
        assert off > 0 and on == off, (B, W, Np, lib.avd_last_error())
        sizes[B, W, Np] = on
    assert len(set(sizes.values())) == 3
