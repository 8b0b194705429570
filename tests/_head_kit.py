"""Scaffolding of tests/test_gpu_noise_head.py: heads whose 1-D parameters are all off their initial values, the fp64 / fp32 CPU chain on
the module's own parameters, the per-row error measure, the inputs, and a ctypes caller of avd_head_forward_f32 that takes the row map
and places the workspace and the output inside sentinel-filled buffers.  Nothing here touches the GPU at import time."""
import ctypes as C
from types import SimpleNamespace

import torch

from oracle import ref_cpu as R

SENT = -12345.5            # the fill of the output buffer and its guard
OUT_GUARD = 1024           # floats after rows * d_out
WS_GUARD = 4096            # bytes after the workspace size that was passed
WS_GUARD_BYTE = 0xA5
NP = 5                     # prompt rows per sample of the segmented buffers (odd: the base pointer row0 * ld is not a multiple of 2 rows)


def make_head(dev, d_in, hidden, d_out, n_shared, n_spec, share, act, seed):
    """MultiModalNoiseHead on the device.  d_out: {modality: width}; every modality reads d_in columns.  Seeded randn * 0.3 is added to
    every 1-D parameter (Linear biases start at 0, LayerNorm weights at 1 and biases at 0: a dropped one would not show otherwise)."""
    import multimodal_diffusion_amd as A
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        head = A.MultiModalNoiseHead({m: d_in for m in d_out}, dict(d_out), hidden_dim=hidden, num_shared_layers=n_shared,
                                     num_modality_specific_layers=n_spec, activation=act, share_parameters=share).eval()
    g = torch.Generator().manual_seed(seed + 1000)
    n_1d = 0
    with torch.no_grad():
        for name, p in head.named_parameters():
            if p.dim() == 1:
                p.add_(torch.randn(p.shape, generator=g) * 0.3)
                assert not ((p == 0) | (p == 1)).any(), name
                n_1d += 1
    assert n_1d >= 2 * len(d_out)
    head.act_name = act
    return head.to(dev)


def head_ref(head, m, x, dtype=torch.float64, trunk_of=None):
    """the chain of modality m on the module's own parameters, on the CPU in `dtype` (float32: the yardstick of the fp32 kernels).
    trunk_of: walk another modality's trunk blocks (a deliberately wrong reference)"""
    p = lambda t: t.detach().cpu().to(dtype)
    act = R._HEAD_ACTS[head.act_name]
    y = R.linear(x.detach().cpu().to(dtype).reshape(-1, x.shape[-1]), p(head.input_proj[m].weight), p(head.input_proj[m].bias))
    for blk in head._trunk(m if trunk_of is None else trunk_of):
        y = R.linear(y, p(blk[0].weight), p(blk[0].bias))
        y = act(R.layernorm(y, p(blk[1].weight), p(blk[1].bias), eps=blk[1].eps))
    return R.linear(y, p(head.out_proj[m].weight), p(head.out_proj[m].bias))


def row_err(y, ref):
    """max over rows of max|y_r - ref_r| / max(1, max|ref_r|); a NaN anywhere in y gives inf"""
    ref = torch.as_tensor(ref, dtype=torch.float64)
    y = torch.as_tensor(y, dtype=torch.float64).reshape(ref.shape)
    if ref.numel() == 0:
        return 0.0
    d = (y - ref).abs().amax(-1)
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    return float((d / ref.abs().amax(-1).clamp(min=1.0)).max())


def make_rows(rows, d_in, seed):
    """randn * 1.7; row 7 times 30, row 1 all zero, row 2 times 1e-3 (where the row count has them)"""
    x = torch.randn(rows, d_in, generator=torch.Generator().manual_seed(seed)) * 1.7
    if rows > 7:
        x[7] *= 30.0
    if rows > 2:
        x[1] = 0.0
        x[2] *= 1e-3
    return x


def bounds(x):
    """(in_bound, in_norm) of weight_table(matmul="f16x2"): max |x_i| and the largest row 2-norm, from the host"""
    x = x.double()
    return float(x.abs().max()), float(x.norm(dim=-1).max())


def seg_buffer(dev, X, S, seg_rows, ld, row0, rows=None):
    """The rows of X as the target rows of a [S, NP + seg_rows, ld] buffer: row r of the call is row row0 + r % seg_rows of sample
    r // seg_rows.  Every other float (the other rows of a sample, the columns past d_in, the rows of the last segment past `rows`, 64
    floats after the last sample) is NaN.  -> (buffer, the view that starts at the first target row, seg_stride)"""
    rows = X.shape[0] if rows is None else rows
    d, N = X.shape[1], NP + seg_rows
    assert rows <= S * seg_rows and ld >= d and row0 in (0, NP)
    buf = torch.full((S * N * ld + 64,), float("nan"))
    full = torch.full((S * seg_rows, d), float("nan"))
    full[:rows] = X[:rows]
    buf[:S * N * ld].view(S, N, ld)[:, row0:row0 + seg_rows, :d] = full.view(S, seg_rows, d)
    assert int(torch.isfinite(buf).sum()) == int(torch.isfinite(X[:rows]).sum())
    buf = buf.to(dev)
    return buf, buf[row0 * ld:], N * ld


def call_head(dev, table, h, rows, *, ldh, seg_rows=0, seg_stride=0, ws_fill=0xFF, ws_bytes=None, out_null=False):
    """avd_head_forward_f32 with the pointer table `table` = head.weight_table(...) (its `keep` stays referenced across the call, as in
    MultiModalNoiseHead.forward).  h: a device tensor whose first element is row 0 (None: a null pointer).  The workspace is
    avd_head_workspace_bytes (or ws_bytes) bytes prefilled with ws_fill, inside a buffer whose next WS_GUARD bytes hold WS_GUARD_BYTE;
    out is [rows, d_out] inside a buffer that holds SENT, with OUT_GUARD more floats behind it.
    -> rc, err (avd_last_error when rc != 0), tags {profiler tag: launches}, out (CPU), untouched (out holds SENT everywhere),
       guards (nothing behind the workspace or behind out was written), need (the workspace size the library asks for)"""
    from multimodal_diffusion_amd import _lib as L
    hw, keep = table
    need = L.lib().avd_head_workspace_bytes(C.byref(hw), rows)
    assert need >= 0, need
    give = need if ws_bytes is None else ws_bytes
    ws = torch.full((give + WS_GUARD,), WS_GUARD_BYTE, dtype=torch.uint8, device=dev)
    ws[:give] = ws_fill
    n_out = rows * hw.d_out
    out = torch.full((n_out + OUT_GUARD,), SENT, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    L.prof_enable(True)
    try:
        rc = L.lib().avd_head_forward_f32(C.byref(hw), None if h is None else h.data_ptr(), ldh, seg_rows, seg_stride, rows,
                                          None if out_null else out.data_ptr(), ws.data_ptr(), give, L.stream_ptr(dev))
        torch.cuda.synchronize()
    finally:
        L.prof_enable(False)
    err = L.lib().avd_last_error().decode("utf-8", "replace") if rc else ""
    tags = {k: v[0] for k, v in L.prof_report().items() if v[0] > 0}
    del keep
    host = out.cpu()
    return SimpleNamespace(rc=rc, err=err, tags=tags, out=host[:n_out].view(rows, hw.d_out), untouched=bool((host == SENT).all()),
                           guards=bool((host[n_out:] == SENT).all()) and bool((ws[give:] == WS_GUARD_BYTE).all()), need=need)


def count(tags, prefix):
    return sum(v for k, v in tags.items() if k.startswith(prefix))
