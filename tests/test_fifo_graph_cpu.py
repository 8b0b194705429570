"""Host side of the graph-replayed FIFO queue: the stacking of the ramp tables the slot-table select reads, the C ABI's new entries,
and what the cursor wrappers refuse before any launch.  ``fifo_denoise``'s own ``graph=`` check sits behind its DenoiseEngine check
and an engine needs a device, so it is covered on the GPU (tests/test_gpu_fifo_graph.py)."""
import re
from pathlib import Path

import pytest
import torch

from multimodal_diffusion_amd import _lib as L
from multimodal_diffusion_amd import functional as Fn
from multimodal_diffusion_amd import schedule_utils as su

NEW = ("avd_cursor_add", "avd_slot_tables_select", "avd_fifo_prompt_gather_f32", "avd_fifo_shift_cursor_f32",
       "avd_fifo_shift_cursor_hist_f32")


@pytest.mark.parametrize("n,S", [(4, 2), (6, 2), (6, 3), (18, 6), (5, 1), (3, 3)])
def test_stacked_ramp_tables_are_the_plan_rows(n, S):
    sched = torch.cat([torch.linspace(999, 0, n).round().long(), torch.tensor([-1])])
    B = n // S
    plan = list(su.fifo_plan(sched, S)[:2]) + [su.fifo_plan_last(sched, S)[0]]
    for rows in plan:
        st = Fn.stack_slot_tables(rows)
        assert st.dtype == torch.long and st.is_contiguous() and tuple(st.shape) == (n - 1, B * S)
        for r in range(n - 1):
            assert torch.equal(st[r].view(B, S), rows[r]), r           # row r is the [B, S] table step_slots takes at ramp step r
    assert torch.equal(Fn.stack_slot_tables(plan[0].to(torch.int32)), Fn.stack_slot_tables(plan[0]))


def test_stack_slot_tables_refusals():
    with pytest.raises(ValueError, match="n_rows, B, S"):
        Fn.stack_slot_tables(torch.zeros(3, 4, dtype=torch.long))
    with pytest.raises(ValueError, match="integer"):
        Fn.stack_slot_tables(torch.zeros(3, 2, 2))
    with pytest.raises(ValueError, match="integer"):
        Fn.stack_slot_tables(torch.zeros(3, 2, 2, dtype=torch.bool))


def test_cursor_entries_are_declared_bound_and_exported():
    header = (Path(__file__).resolve().parent.parent / "include" / "avdiff_hip.h").read_text()
    declared = set(re.findall(r"\b(avd_[a-z0-9_]+)\s*\(", header))
    lib = L.lib()
    for name in NEW:
        assert name in declared and name in L.SIGNATURES and hasattr(lib, name), name
    assert set(L.SIGNATURES) == declared
    assert lib.avd_abi_version() == L.ABI_VERSION == 7
    assert "FIFO device cursors" in header and "FIFO queue shift off a device cursor" in header


def test_cursor_wrappers_refuse_host_tensors_before_any_launch():
    cursor = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="cursor"):
        Fn.cursor_add(cursor)
    with pytest.raises(ValueError, match="prompt canvas"):
        Fn.fifo_prompt_gather(torch.zeros(8, 150), cursor, 2, 2, 20, 40)
    with pytest.raises(ValueError, match="two or three"):
        Fn.slot_tables_select([torch.zeros(3, 4, dtype=torch.long)], cursor, [torch.zeros(4, dtype=torch.long)])
    with pytest.raises(ValueError, match="device tensors"):
        Fn.slot_tables_select([torch.zeros(3, 4, dtype=torch.long)] * 2, cursor, [torch.zeros(4, dtype=torch.long)] * 2)
    with pytest.raises(L.AvdError, match="ROCm device"):
        Fn.fifo_shift_cursor(torch.zeros(2, 8, 40), 4, cursor, torch.zeros(8, 16), 5, 999, 4)
