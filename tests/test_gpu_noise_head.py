"""The noise head at the C ABI (avd_head_forward_f32: head_forward in csrc/composite.hip), on heads whose biases and LayerNorm
parameters are all off their initial values, against the fp64 chain on the module's own parameters (tests/_head_kit.py).

A. trunk and width variants on the fp32 kernels (matmul "f32"), rows 1 and 300, both modalities, through the module and through the ABI:
   128/64 -> 256|32 trunk 2 gelu; 512/512 -> 256|32 trunk 2 gelu; 1024/256 -> 512|48 trunk 0 relu; 192/768 -> 256|40 shared 1 + two
   spec.{m} blocks, leaky_relu; 64/256 -> 256|16 the shared-specific trunk (one block), gelu.  rows == 0: nothing launched.
B. segmented rows on the fp32 kernels: [S, 5 + seg_rows, ld] buffers, ld in {d_in, d_in + 4, d_in + 36}, target rows first or after the
   five prompt rows, NaN everywhere else; (S, seg_rows) in (3, 1), (7, 5), (4, 24), (3, 37), (2, 130), (1, 300), and (7, 5) with 32 rows
   (the last segment ends early); gemm_tile default, 0, 1, 2; heads 512/512 -> 256 trunk 2 and 128/64 -> 32 (register kernel).  Bit
   identity with the contiguous call, guards, workspace prefilled with 0xFF and 0x00 bytes.
C. the split-operand head ("s3_min_rows" 0) in the modes bf16x3, bf16x3_strict, f16x2, bf16, rows 1, 255, 257, 300: 512/512 -> 256 with
   trunk 0, 1, 2, 3; 1024/256 -> 512 trunk 1 (the images are d_in wide); 48/768 -> 256 trunk 2.  Which kernels ran (profiler tags),
   error, workspace poisoning, one segmented call, row locality; the 6,143 / 6,144-row threshold at default keys; the f16x2 scale table.
D. workspace sizes and the refusals the host makes before a launch.

Tolerances.  fp32 kernels: e < K_F32 * e_cpu + 1e-7, where e = row_err against fp64 and e_cpu is the row_err of the same chain run in fp32
on the CPU (the arithmetic's own error, computed in the test for the same head and input).  bf16x3, bf16x3_strict, f16x2: e < 3 * e32 +
1e-7 (test_head_split_modes_vs_oracle's rule), e32 the fp32 kernels' error on the same input, itself held to the first rule.  bf16 (one
term): reported, e > e32, and e < 2 x the value measured on the MI355X (BF16_MEASURED).  Bit identity, guards, poisoning and row
locality have no tolerance.

What the module found.  A: MultiModalNoiseHead.forward handed the library null pointers for an empty batch (an empty tensor has no
storage) and raised "head: null pointer"; it now returns the empty output without a call.  A / C, row locality: the ReLU of
layernorm_act_kernel and layernorm_act_split3_kernel was fmaxf(t, 0), which returns 0 for NaN, so behind the first trunk block of a ReLU
head a NaN input row came out as an ordinary finite row (nn.ReLU keeps NaN; in f16x2 it also hid a value past the fp16 range).  B and D
found nothing.  The module runs in about 2.5 s on the MI355X."""
import ctypes as C
from functools import lru_cache

import pytest
import torch

from _head_kit import NP, bounds, call_head, count, head_ref, make_head, make_rows, row_err, seg_buffer
from _kit import dev  # noqa: F401  (fixture)
from _tune import tuned

gpu = pytest.mark.gpu

# e / e_cpu observed on the MI355X, the largest of each section (the tests print every ratio): A 2.72 (64/256 audio, 1 row), B 2.77
# (512/512 video, 7 segments of 5 rows; the same on every tile), the fp32 runs of C 2.68 (48/768, 255 rows); the smallest 0.81.
# K_F32 = twice the largest of A and B, rounded up to an integer (the rule allows at most 8).
K_F32_OBSERVED = 2.77
K_F32 = 6
# bf16 (one product term): largest row_err against fp64 measured on the MI355X over rows 1, 255, 257, 300, per head of C; the bound is
# twice this.  (The fp32 kernels' error on the same inputs: 4.8e-7 to 1.7e-6.)
BF16_MEASURED = {"512_t0": 5.547e-3, "512_t1": 6.770e-3, "512_t2": 8.493e-3, "512_t3": 7.298e-3, "1024x256_t1": 6.114e-3,
                 "48x768_t2": 6.190e-3}

SPLIT = "gemm_bf16x3"          # prefix of every tag launch_s3w / launch_s3w16 / launch_s3w128 register (csrc/gemm_bf16x3.hip)
F32 = "gemm_f32"               # ... launch_dma / launch_reg_k (csrc/gemm_f32.hip)
IMAGE_TAGS = {"split3_kernel", "layernorm_act_split3_kernel"}
MODES = ["bf16x3", "bf16x3_strict", "f16x2", "bf16"]

# name: d_in, hidden, {modality: d_out}, shared, modality-specific, share_parameters, activation, seed
HEADS_A = {"128x64": (128, 64, {"video": 256, "audio": 32}, 2, 1, False, "gelu", 11),
           "512x512": (512, 512, {"video": 256, "audio": 32}, 2, 1, False, "gelu", 12),
           "1024x256_t0": (1024, 256, {"video": 512, "audio": 48}, 0, 1, False, "relu", 13),
           "192x768_spec": (192, 768, {"video": 256, "audio": 40}, 1, 3, False, "leaky_relu", 14),
           "64x256_shared_spec": (64, 256, {"video": 256, "audio": 16}, 0, 2, True, "gelu", 15)}
TRUNK_A = {"128x64": 2, "512x512": 2, "1024x256_t0": 0, "192x768_spec": 3, "64x256_shared_spec": 1}
HEADS_C = {"512_t0": (512, 512, {"video": 256, "audio": 32}, 0, 1, False, "gelu", 20),
           "512_t1": (512, 512, {"video": 256, "audio": 32}, 1, 1, False, "gelu", 21),
           "512_t2": (512, 512, {"video": 256, "audio": 32}, 2, 1, False, "gelu", 22),
           "512_t3": (512, 512, {"video": 256, "audio": 32}, 3, 1, False, "leaky_relu", 23),
           "1024x256_t1": (1024, 256, {"video": 512, "audio": 32}, 1, 1, False, "gelu", 24),
           "48x768_t2": (48, 768, {"video": 256, "audio": 32}, 2, 1, False, "relu", 25)}
TRUNK_C = {"512_t0": 0, "512_t1": 1, "512_t2": 2, "512_t3": 3, "1024x256_t1": 1, "48x768_t2": 2}
HEADS = {**HEADS_A, **HEADS_C}
SEGS = [(3, 1, None), (7, 5, None), (7, 5, 32), (4, 24, None), (3, 37, None), (2, 130, None), (1, 300, None)]      # S, seg_rows, rows

_heads = {}


def head_of(dev, name):
    """the head `name`, built once for the module (matmul "f32": the module's own calls stay on the fp32 kernels)"""
    if name not in _heads:
        _heads[name] = make_head(dev, *HEADS[name])
        _heads[name].matmul = "f32"
    return _heads[name]


@lru_cache(maxsize=None)
def _rows_of(d_in, rows):
    return make_rows(rows, d_in, seed=1000 + rows)


_refs = {}


def case(dev, name, m, rows):
    """(x [rows, d_in] on the CPU, fp64 reference, e_cpu): built once per head, modality and row count, never modified"""
    key = (name, m, rows)
    if key not in _refs:
        head = head_of(dev, name)
        x = _rows_of(HEADS[name][0], rows)
        ref = head_ref(head, m, x)
        _refs[key] = (x, ref, row_err(head_ref(head, m, x, dtype=torch.float32), ref))
    return _refs[key]


def table(head, m, mode, x):
    if mode == "f16x2":
        b, n = bounds(x)
        return head.weight_table(m, matmul=mode, in_bound=b, in_norm=n)
    return head.weight_table(m, matmul=mode)


def ok(r):
    assert r.rc == 0, r.err
    assert r.guards, "written behind the workspace or behind out"
    return r


def check_f32(what, out, ref, e_cpu):
    """the fp32 kernels' rule; -> e"""
    e = row_err(out, ref)
    print(f"{what}: e {e:.3e}  e_cpu {e_cpu:.3e}  ratio {e / e_cpu if e_cpu else float('nan'):.2f}")
    assert torch.isfinite(out).all()
    assert e < K_F32 * e_cpu + 1e-7, (what, e, e_cpu)
    return e


def same(a, b, what):
    bad = ((a != b) | torch.isnan(a) | torch.isnan(b)).nonzero()
    assert torch.equal(a, b), f"{what}: {len(bad)} elements differ, rows {bad[:, 0].unique().tolist()[:12]}"


def check_row_locality(dev, tab, x, rows, base, what):
    """one input row replaced by NaN: that output row is non-finite in every column, every other row keeps its bits"""
    bad = 5 if rows > 5 else 0
    xn = x.clone()
    xn[bad] = float("nan")
    rn = ok(call_head(dev, tab, xn.to(dev), rows, ldh=x.shape[1]))
    rest = torch.arange(rows) != bad
    assert not torch.isfinite(rn.out[bad]).any(), f"{what}: the output row of a NaN input row has finite values"
    same(rn.out[rest], base[rest], f"{what}: the rows beside a NaN input row")


def f32_tags_only(tags, trunk):
    assert count(tags, F32) == trunk + 2 and not count(tags, SPLIT) and not (IMAGE_TAGS & set(tags)), tags


def split_tags_only(tags, trunk):
    assert count(tags, SPLIT) == trunk + 2 and not count(tags, F32), tags
    assert tags.get("split3_kernel") == 1 and tags.get("layernorm_act_split3_kernel", 0) == trunk, tags
    assert all(k.startswith(SPLIT) or k in IMAGE_TAGS for k in tags), tags


# ------------------------------------------------------------------------------------------------- the tables, without a GPU
def test_head_tables_build_what_they_claim():
    cpu = torch.device("cpu")
    for names, trunks in ((HEADS_A, TRUNK_A), (HEADS_C, TRUNK_C)):
        for name in names:
            head = make_head(cpu, *HEADS[name])
            for m in head.modalities:
                assert len(head._trunk(m)) == trunks[name], (name, m)
    spec = make_head(cpu, *HEADS["192x768_spec"])
    assert [id(b) for b in spec._trunk("video")[1:]] != [id(b) for b in spec._trunk("audio")[1:]]
    assert spec._trunk("video")[0] is spec._trunk("audio")[0]
    shared = make_head(cpu, *HEADS["64x256_shared_spec"])
    assert shared._trunk("video")[0] is shared._trunk("audio")[0] and shared.shared is None
    for name, (d_in, hidden, d_out, *_) in HEADS_C.items():
        assert hidden % 256 == 0 and d_out["video"] % 256 == 0 and d_in % 16 == 0 and d_out["audio"] == 32
    assert {t % 2 for t in TRUNK_C.values()} == {0, 1} and 0 in TRUNK_C.values()


# ------------------------------------------------------------------------------------------------- A
@gpu
@pytest.mark.parametrize("m", ["video", "audio"])
@pytest.mark.parametrize("rows", [1, 300])
@pytest.mark.parametrize("name", list(HEADS_A))
def test_trunk_and_width_variants_f32(dev, name, rows, m):
    head = head_of(dev, name)
    x, ref, e_cpu = case(dev, name, m, rows)
    xd = x.to(dev)
    r = ok(call_head(dev, head.weight_table(m, matmul="f32"), xd, rows, ldh=x.shape[1]))
    f32_tags_only(r.tags, TRUNK_A[name])
    check_f32(f"A {name} {m} rows {rows}", r.out, ref, e_cpu)
    check_row_locality(dev, head.weight_table(m, matmul="f32"), x, rows, r.out, "f32")
    same(head({m: xd})[m].cpu(), r.out, "the module's call against the ABI call")


@gpu
def test_spec_blocks_run_per_modality(dev):
    """192/768: video and audio share shared.0 and then run their own two spec blocks"""
    head = head_of(dev, "192x768_spec")
    x, _, _ = case(dev, "192x768_spec", "video", 300)
    out = head({"video": x.to(dev), "audio": x.to(dev)})
    v, a = out["video"].cpu(), out["audio"].cpu()
    assert not torch.equal(v[:, :40], a)
    # each output fits its own trunk (test above) and is far from the chain that walks the other modality's blocks
    assert row_err(v, head_ref(head, "video", x, trunk_of="audio")) > 1e-2
    assert row_err(a, head_ref(head, "audio", x, trunk_of="video")) > 1e-2


@gpu
@pytest.mark.parametrize("name", ["512x512", "1024x256_t0", "512_t2"])
def test_zero_rows_launch_nothing(dev, name):
    from multimodal_diffusion_amd import _lib as L
    head = head_of(dev, name)
    d_in = HEADS[name][0]
    some = torch.zeros(4, d_in, device=dev)
    for mode in ("f32", "bf16x3"):
        with tuned(s3_min_rows=0):
            r = ok(call_head(dev, head.weight_table("video", matmul=mode), some, 0, ldh=d_in))
        assert r.need == 0 and r.tags == {} and r.untouched, (mode, r.tags)
    L.prof_enable(True)
    try:
        out = head({"video": torch.empty(0, d_in, device=dev), "audio": torch.empty(2, 0, d_in, device=dev)})
        torch.cuda.synchronize()
    finally:
        L.prof_enable(False)
    assert {k: v[0] for k, v in L.prof_report().items() if v[0] > 0} == {}
    assert out["video"].shape == (0, HEADS[name][2]["video"]) and out["audio"].shape == (2, 0, HEADS[name][2]["audio"])


# ------------------------------------------------------------------------------------------------- B
@gpu
@pytest.mark.parametrize("S,seg_rows,n_rows", SEGS)
@pytest.mark.parametrize("name,m", [("512x512", "video"), ("128x64", "audio")])
def test_segmented_rows_f32(dev, name, m, S, seg_rows, n_rows):
    head = head_of(dev, name)
    rows = S * seg_rows if n_rows is None else n_rows
    assert S * seg_rows - seg_rows < rows <= S * seg_rows
    x, ref, e_cpu = case(dev, name, m, rows)
    d_in = x.shape[1]
    xd = x.to(dev)
    tab = head.weight_table(m, matmul="f32")
    for tile in (None, 0, 1, 2):
        with tuned(**({} if tile is None else {"gemm_tile": tile})):
            flat = ok(call_head(dev, tab, xd, rows, ldh=d_in))
            f32_tags_only(flat.tags, TRUNK_A[name])
            check_f32(f"B {name} {m} S {S} seg {seg_rows} rows {rows} tile {tile}", flat.out, ref, e_cpu)
            same(ok(call_head(dev, tab, xd, rows, ldh=d_in, ws_fill=0x00)).out, flat.out, "workspace prefilled with 0x00 against 0xFF")
            for ld in (d_in, d_in + 4, d_in + 36):
                for row0 in (0, NP):
                    buf, h, stride = seg_buffer(dev, x, S, seg_rows, ld, row0, rows)
                    what = f"tile {tile} ld {ld} row0 {row0}"
                    r = ok(call_head(dev, tab, h, rows, ldh=ld, seg_rows=seg_rows, seg_stride=stride))
                    assert r.tags == flat.tags, (what, r.tags, flat.tags)
                    same(r.out, flat.out, f"segmented against contiguous, {what}")
                    if tile is None:
                        r0 = ok(call_head(dev, tab, h, rows, ldh=ld, seg_rows=seg_rows, seg_stride=stride, ws_fill=0x00))
                        same(r0.out, flat.out, f"segmented, workspace prefilled with 0x00, {what}")


# ------------------------------------------------------------------------------------------------- C
@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(HEADS_C))
def test_split_head_small_sizes(dev, name, mode):
    head = head_of(dev, name)
    d_in, trunk = HEADS[name][0], TRUNK_C[name]
    worst = 0.0
    for rows in (1, 255, 257, 300):
        x, ref, e_cpu = case(dev, name, "video", rows)
        xd = x.to(dev)
        r32 = ok(call_head(dev, head.weight_table("video", matmul="f32"), xd, rows, ldh=d_in))
        f32_tags_only(r32.tags, trunk)
        e32 = check_f32(f"C {name} f32 rows {rows}", r32.out, ref, e_cpu)
        check_row_locality(dev, head.weight_table("video", matmul="f32"), x, rows, r32.out, f"f32 rows {rows}")
        with tuned(s3_min_rows=0):
            tab = table(head, "video", mode, x)
            r = ok(call_head(dev, tab, xd, rows, ldh=d_in))
            split_tags_only(r.tags, trunk)
            assert torch.isfinite(r.out).all()
            e = row_err(r.out, ref)
            print(f"C {name} {mode} rows {rows}: e {e:.3e}  e32 {e32:.3e}")
            if mode == "bf16":
                worst = max(worst, e)
                assert e > e32, (e, e32)
            else:
                assert e < 3.0 * e32 + 1e-7, (e, e32)
            # the images' rows past `rows` (up to the next multiple of 256) are never written: a 256-row tile reads them as A operands
            same(ok(call_head(dev, tab, xd, rows, ldh=d_in, ws_fill=0x00)).out, r.out, f"rows {rows}: workspace prefilled with 0x00 against 0xFF")
            check_row_locality(dev, tab, x, rows, r.out, f"{mode} rows {rows}")
    if mode == "bf16":
        print(f"C {name} bf16: largest e {worst:.3e}")
        assert worst < 2.0 * BF16_MEASURED[name], (worst, BF16_MEASURED[name])
    # split3_rows_f32 with a row map, NaN around the rows
    S, seg_rows, rows = 3, 37, 111
    x, ref, _ = case(dev, name, "video", rows)
    with tuned(s3_min_rows=0):
        tab = table(head, "video", mode, x)
        flat = ok(call_head(dev, tab, x.to(dev), rows, ldh=d_in))
        split_tags_only(flat.tags, trunk)
        buf, h, stride = seg_buffer(dev, x, S, seg_rows, d_in + 36, NP)
        r = ok(call_head(dev, tab, h, rows, ldh=d_in + 36, seg_rows=seg_rows, seg_stride=stride))
        assert r.tags == flat.tags
        same(r.out, flat.out, "segmented against contiguous")
        # the audio path of the same head (d_out = 32) stays on the fp32 kernels
        xa, _, _ = case(dev, name, "audio", 300)
        ra = ok(call_head(dev, table(head, "audio", mode, xa), xa.to(dev), 300, ldh=d_in))
        f32_tags_only(ra.tags, trunk)
    same(ra.out, ok(call_head(dev, head.weight_table("audio", matmul="f32"), xa.to(dev), 300, ldh=d_in)).out, "audio path against f32")


@gpu
def test_split_threshold_at_default_keys(dev):
    """512/512 -> 256, trunk 2, bf16x3: 6,143 rows stay on the fp32 kernels, 6,144 take the split kernels"""
    head = head_of(dev, "512_t2")
    e32 = {}
    for rows in (6143, 6144):
        x, ref, e_cpu = case(dev, "512_t2", "video", rows)
        xd = x.to(dev)
        r32 = ok(call_head(dev, head.weight_table("video", matmul="f32"), xd, rows, ldh=512))
        f32_tags_only(r32.tags, 2)
        e32[rows] = check_f32(f"C threshold f32 rows {rows}", r32.out, ref, e_cpu)
        r = ok(call_head(dev, head.weight_table("video", matmul="bf16x3"), xd, rows, ldh=512))
        if rows == 6143:
            f32_tags_only(r.tags, 2)
            same(r.out, r32.out, "below the threshold: the fp32 kernels")
        else:
            split_tags_only(r.tags, 2)
            e = row_err(r.out, ref)
            print(f"C threshold bf16x3 rows {rows}: e {e:.3e}  e32 {e32[rows]:.3e}")
            assert e < 3.0 * e32[rows] + 1e-7, (e, e32[rows])


@gpu
def test_f16x2_scale_table(dev):
    head = head_of(dev, "512_t2")
    rows, n = 300, 2
    x, ref, _ = case(dev, "512_t2", "video", rows)
    xd = x.to(dev)
    r32 = ok(call_head(dev, head.weight_table("video", matmul="f32"), xd, rows, ldh=512))
    with tuned(s3_min_rows=0):
        for i in (0, n + 1, n + 2, 2 * (n + 2) - 1):
            for v in (0.0, -4.0, float("inf")):
                hw, keep = table(head, "video", "f16x2", x)
                good = hw.f16x2_scale[i]
                assert good > 0
                hw.f16x2_scale[i] = v
                r = call_head(dev, (hw, keep), xd, rows, ldh=512)
                hw.f16x2_scale[i] = good          # the module caches the Python list, not this array; put back all the same
                assert r.rc == -1 and r.err == f"head: f16x2_scale[{i}] must be positive and finite", (r.rc, r.err)
                assert r.untouched and r.guards and r.tags == {}
        hw, keep = table(head, "video", "f16x2", x)
        hw.f16x2_scale = C.POINTER(C.c_float)()
        r = ok(call_head(dev, (hw, keep), xd, rows, ldh=512))
        f32_tags_only(r.tags, 2)
        same(r.out, r32.out, "a null scale table: the fp32 kernels")


@gpu
def test_f16x2_value_past_the_range_is_nan(dev):
    """include/avdiff_hip.h: "a value past the range turns its output rows into NaN, never into a silently saturated number".
    Row 9 is scaled up until the largest of the other rows' values is below 1/64 of its maximum; in_bound = that maximum / 64.
    (a) randn rows: every other row has the bits of a run with the same bound in which row 9 fits it (scaled down by 2^-7).
    (b) the bits of the run with the true maximum as the bound: an image scale 64 times smaller.  An fp16 pair holds all 22 bits only of
        values within 18 binades of the top of the range, so for this comparison the rows are multiples of 1/16 below 8 (eight significant
        bits: the high plane holds them exactly at either scale) — every image element is then the same number in both runs."""
    head = head_of(dev, "512_t2")
    rows = 300
    with tuned(s3_min_rows=0):
        for exact in (False, True):
            x = make_rows(rows, 512, seed=77)
            if exact:
                x = (x.clamp(-7.9, 7.9) * 16).round() / 16
            rest = torch.arange(rows) != 9
            x[9] *= 2.0 ** 12
            top = float(x[9].abs().max())
            bound, norm = top / 64, bounds(x)[1]
            assert float(x[rest].abs().max()) * 1.01 <= bound and (x[9].abs() * 1.01 > bound * 2).any()
            short = head.weight_table("video", matmul="f16x2", in_bound=bound, in_norm=norm)
            r = ok(call_head(dev, short, x.to(dev), rows, ldh=512))
            split_tags_only(r.tags, 2)
            assert not torch.isfinite(r.out[9]).any(), "the row past the range must be non-finite in every column"
            assert torch.isfinite(r.out[rest]).all()
            if exact:
                right = head.weight_table("video", matmul="f16x2", in_bound=top, in_norm=norm)
                assert right[0].f16x2_scale[4] * 64 == short[0].f16x2_scale[4]
                good = ok(call_head(dev, right, x.to(dev), rows, ldh=512))
                assert torch.isfinite(good.out).all()
            else:
                xs = x.clone()
                xs[9] *= 2.0 ** -7
                assert float(xs.abs().max()) * 1.01 <= bound
                good = ok(call_head(dev, head.weight_table("video", matmul="f16x2", in_bound=bound, in_norm=norm), xs.to(dev), rows, ldh=512))
                assert torch.isfinite(good.out).all()
                assert row_err(good.out[rest], head_ref(head, "video", x[rest])) < 1e-5
            same(r.out[rest], good.out[rest], f"rows beside the row past the range (exact={exact})")


# ------------------------------------------------------------------------------------------------- D
@gpu
@pytest.mark.parametrize("name", ["512_t2", "1024x256_t1", "48x768_t2", "128x64"])
def test_workspace_sizes(dev, name):
    from multimodal_diffusion_amd import _lib as L
    head = head_of(dev, name)
    d_in = HEADS[name][0]
    rows = 300
    x, ref, _ = case(dev, name, "video", rows)
    xd = x.to(dev)
    t32 = head.weight_table("video", matmul="f32")
    need32 = L.lib().avd_head_workspace_bytes(C.byref(t32[0]), rows)
    assert L.lib().avd_head_workspace_bytes(None, rows) == -1 and L.lib().avd_head_workspace_bytes(C.byref(t32[0]), -1) == -1
    assert L.lib().avd_head_workspace_bytes(C.byref(t32[0]), 0) == 0
    r32 = ok(call_head(dev, t32, xd, rows, ldh=d_in))
    for mode in ["f32"] + (MODES if name in HEADS_C else []):
        tab = table(head, "video", mode, x)
        need = L.lib().avd_head_workspace_bytes(C.byref(tab[0]), rows)        # sized with "s3_min_rows" at its default
        assert need >= need32 > 0
        for min_rows in (0, 10 ** 9):
            with tuned(s3_min_rows=min_rows):
                r = ok(call_head(dev, tab, xd, rows, ldh=d_in))
                assert r.need == need
                if mode == "f32" or min_rows:
                    same(r.out, r32.out, f"{mode} at s3_min_rows {min_rows}: the fp32 kernels")
                else:
                    assert count(r.tags, SPLIT) and torch.isfinite(r.out).all()
                short = call_head(dev, tab, xd, rows, ldh=d_in, ws_bytes=need - 1)
                assert short.rc == L.EWORKSPACE and short.err == "head: workspace too small", (short.rc, short.err)
                assert short.untouched and short.guards and short.tags == {}


@gpu
def test_argument_refusals(dev):
    from multimodal_diffusion_amd import _lib as L
    head = head_of(dev, "512_t2")
    rows, S, seg_rows = 35, 7, 5
    x, _, _ = case(dev, "512_t2", "video", rows)
    xd = x.to(dev)

    def refused(rc, text, tab, h=xd, exact=True, **kw):
        kw.setdefault("ldh", 512)
        r = call_head(dev, tab, h, rows, **kw)
        assert r.rc == rc and (r.err == text if exact else text in r.err), (r.rc, r.err)
        assert r.untouched and r.guards and r.tags == {}

    def patched(mode="f32", **fields):
        hw, keep = head.weight_table("video", matmul=mode)
        for k, v in fields.items():
            setattr(hw, k, v)
        return hw, keep

    null_table = C.POINTER(C.c_void_p)()
    refused(L.EINVAL, "head: null pointer", patched(), h=None)
    refused(L.EINVAL, "head: null pointer", patched(), out_null=True)
    refused(L.EINVAL, "head: null weights", patched(input_proj_weight=None))
    refused(L.EINVAL, "head: null weights", patched(out_proj_weight=None))
    refused(L.EINVAL, "head: split_terms must be 0 (fp32), 6, 9, 1 or 3, got 5", patched(split_terms=5))
    for f in ("shared_lin_weight", "shared_lin_bias", "shared_ln_weight", "shared_ln_bias"):
        refused(L.EINVAL, "head: null shared-trunk tables", patched(**{f: null_table}))
    # row strides that are no multiple of 4 floats: the first kernel's launcher refuses (fp32 GEMM / split3 producer)
    buf, h, stride = seg_buffer(dev, x, S, seg_rows, 512 + 4, NP)
    for mode, min_rows, text in (("f32", 10 ** 9, "gemm: A row stride must be a multiple of 4 floats"), ("bf16x3", 0, "split3: need ")):
        with tuned(s3_min_rows=min_rows):
            refused(L.EUNSUPPORTED, text, patched(mode), h=h, exact=mode == "f32", ldh=512 + 2, seg_rows=seg_rows, seg_stride=stride)
            refused(L.EUNSUPPORTED, text, patched(mode), h=h, exact=mode == "f32", ldh=512 + 4, seg_rows=seg_rows, seg_stride=stride + 2)
            refused(L.EUNSUPPORTED, text, patched(mode), h=h, exact=mode == "f32", ldh=512 + 2)
