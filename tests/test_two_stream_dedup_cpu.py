"""CPU-only checks around the two-stream short null layout (no GPU, no kernel launches): the "cfg_offset" tune key's range and the step's
workspace plan under every split_streams value."""
import ctypes as C

from test_null_dedup_cpu import _tables

OFFSET_DEFAULT = 0          # g_cfg_offset in csrc/composite.hip


def test_cfg_offset_takes_zero_to_three():
    from multimodal_diffusion_amd import _lib as L
    lib = L.lib()
    try:
        for k in (0, 1, 2, 3):
            assert lib.avd_tune_set(b"cfg_offset", k) == 0, k
        for bad in (-1, 4, 1 << 40):
            assert lib.avd_tune_set(b"cfg_offset", bad) == L.EINVAL, bad
            assert b"cfg_offset" in lib.avd_last_error()
    finally:
        assert lib.avd_tune_set(b"cfg_offset", OFFSET_DEFAULT) == 0


def test_workspace_plan_does_not_depend_on_the_stream_layout():
    """the halves of the short two-stream form live in the halves of the plan that the full two-stream form has: nothing grows"""
    from multimodal_diffusion_amd import _lib as L
    lib = L.lib()
    blocks, core, head = _tables(L)
    for B, W, Np in ((2, 48, 2), (3, 32, 37), (32, 64, 37)):
        s = L.StepDesc()
        e = s.embed
        e.target_kind, e.target_first, e.B, e.d, e.tdim = 0, 1, B, 512, 256
        e.C, e.T, e.H, e.W, e.p0, e.p1, e.p2 = 8, 4, 16, W, 2, 4, 4
        e.Nt, e.Np = 2 * 4 * (W // 4), Np
        s.core, s.head = C.pointer(core), C.pointer(head)
        s.T_train, s.guidance = 1000, 3.5
        sizes = []
        for split in (0, 1, 2):
            s.split_streams = split
            sizes.append(lib.avd_step_workspace_bytes(C.byref(s)))
        assert sizes[0] > 0 and sizes[1] == sizes[0] and sizes[2] == sizes[0], (B, W, Np, sizes, lib.avd_last_error())
