"""Which kernel the split-operand GEMM host code picks (csrc/gemm_bf16x3.hip: launch_s3t and the split-K plan), pinned through the
profiling tags.  Every case is one call of one entry at row counts one block either side of each threshold in the host rules, computed
from those rules for a 256-CU device; EXPECT holds the tags each case ran, recorded on the commit before the launch ladders were
collapsed.  Outputs are not checked here (tests/test_gpu_parity.py and tests/test_gpu_f16x2.py do that): the operand images are zeros."""
import pytest
import torch

from _tune import tuned

pytestmark = pytest.mark.gpu

CU = 256


# ---- the host rules, restated (rows either side of a change of these functions are the cases) ----
def _cdiv(a, b):
    return (a + b - 1) // b


def _rt4_for(M, N, rt_min):
    """s3_rt4_for, automatic: rows per 4-wave block / 32"""
    best, cost8, cbest = 8, 0, 0
    for rt in range(8, rt_min - 1, -1):
        cost = _cdiv(_cdiv(M, 32 * rt) * (N // 128), CU) * (rt + 3)
        if rt == 8:
            cost8 = cbest = cost
        elif cost < cbest:
            cbest, best = cost, rt
    return best if cbest * 100 <= cost8 * 94 else 8


def _rows8_for(M, N):
    """the 192 / 224 / 256-row choice of the residual + image epilogue (one block per CU), automatic"""
    g8, g7, g6 = (_cdiv(_cdiv(M, 32 * rt) * (N // 256), CU) * rt for rt in (8, 7, 6))
    return 6 if g6 < g7 and g6 < g8 else 7 if g7 < g8 else 8


def _changes(fn, lo, hi, most=6):
    """row counts M, M + 1 around the first `most` places in [lo, hi) where fn(M) != fn(M + 1) (blocks start at multiples of 32 rows)"""
    out = []
    for M in range(lo - lo % 32 + 32, hi, 32):
        if fn(M) != fn(M + 1):
            out += [M, M + 1]
            if len(out) >= 2 * most:
                break
    return out


def _rows(N, rt_min, eight_wave):
    nbn = N // 128
    tile = 256 * (_cdiv(192, N // 256) - 1)                   # s3_tile_for: 192 blocks of 256 x 256
    ms = {1, 300, tile, tile + 1}
    for rt in range(2, 9):                                      # the blocks fit the CUs once
        ms |= {32 * rt * (CU // nbn), 32 * rt * (CU // nbn) + 1}
    ms |= set(_changes(lambda M: _rt4_for(M, N, rt_min), 32, tile))       # the 6 % rule
    if eight_wave:
        ms |= set(_changes(lambda M: _rows8_for(M, N), tile, tile + 16384))
    return sorted(ms)


FORCED = [dict(s3_tile=0), dict(s3_tile=1), dict(s3_m16=0), dict(s3_w128=0), dict(s3_rt=7), dict(s3_rt=8), dict(s3_deep4=0),
          dict(s3_tile=0, s3_rt=7, s3_w128=0)] + [dict(s3_rt4=rt) for rt in range(2, 9)]
LINEAR = {"bias": dict(bias=True), "residual": dict(bias=True, residual=True), "gelu_image": dict(bias=True, gelu=True, image=True),
          "image": dict(bias=True, image=True)}


def _cases():
    """(entry, terms, M, N, K, tune keys) -> id string"""
    out = []
    for entry in LINEAR:
        rt_min = 5 if entry == "gelu_image" else 2
        for N in (256, 512, 2048) if entry == "gelu_image" else (256, 512):
            for M in _rows(N, rt_min, entry == "residual"):
                out.append((entry, 6, M, N, 512, {}))
        for M in (300, 4097, 24321):
            out += [(entry, 6, M, 512, 512, keys) for keys in FORCED]
            out += [(entry, terms, M, 512, K, {}) for terms in (9, 1, 3) for K in (512, 1024)]
            out.append((entry, 6, M, 512, 1024, {}))
    for N in (1536,):
        out += [("qkv3", 6, M, N, 512, {}) for M in _rows(N, 5, False)]
        for M in (300, 4097, 24321):
            out += [("qkv3", 6, M, N, 512, keys) for keys in FORCED]
            out += [("qkv3", terms, M, N, K, {}) for terms in (9, 1, 3) for K in (512, 1024)]
    # one MMDiT layer (d = 512): out_proj / fc2 in the residual + image + sums-of-squares epilogue, fc2 through split-K where it applies
    # (K = the MLP's hidden width: 1,024 allows two slices, 2,048 four); s3_min_rows 0 keeps small row counts on the split kernels
    for terms in (6, 9, 1, 3):
        for K in (1024, 2048):
            rows = {300, 4096, 4097, 8192, 8193, 24320, 24321}           # split-K: blocks x slices x 2 <= CUs, then the 192-block rule
            if terms == 6 and K == 2048:
                rows |= set(_rows(512, 2, True))
            out += [("core", terms, M, 512, K, dict(s3_min_rows=0)) for M in sorted(rows)]
            for M in (4097, 24321):
                out += [("core", terms, M, 512, K, dict(s3_min_rows=0, s3_splitk=ns)) for ns in (0, 2)]
                if terms == 6:
                    out += [("core", terms, M, 512, K, dict(s3_min_rows=0, **keys)) for keys in FORCED]
    return out


def _case_id(case):
    entry, terms, M, N, K, keys = case
    return f"{entry} t{terms} M{M} N{N} K{K}" + "".join(f" {k}={v}" for k, v in sorted(keys.items()))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if torch.cuda.get_device_properties(0).multi_processor_count != CU:
        pytest.skip(f"the thresholds are computed for {CU} CUs")
    return torch.device("cuda:0")


class _Runner:
    """runs one case and returns the sorted GEMM tags with a non-zero launch count"""

    def __init__(self, dev):
        from multimodal_diffusion_amd import _lib as L
        self.dev, self.L, self.lib = dev, L, L.lib()
        self.buf = {}
        self.cores = {}

    def zeros(self, name, nbytes):
        if name not in self.buf or self.buf[name].numel() < nbytes:
            self.buf[name] = torch.zeros(nbytes, dtype=torch.uint8, device=self.dev)
        return self.buf[name]

    def core(self, hidden):
        import multimodal_diffusion_amd as A
        if hidden not in self.cores:
            torch.manual_seed(hidden)
            self.cores[hidden] = A.MMDiT(d_model=512, n_layers=1, n_heads=8, mlp_ratio=hidden / 512).to(self.dev).eval()
        return self.cores[hidden]

    def launch(self, entry, terms, M, N, K):
        L, lib, st = self.L, self.lib, self.L.stream_ptr(self.dev)
        if entry == "core":
            core = self.core(K)
            core.matmul = {6: "bf16x3", 9: "bf16x3_strict", 1: "bf16", 3: "f16x2"}[terms]
            tokens = max(n for n in range(1, 1025) if M % n == 0)
            tokens = tokens if tokens >= 64 else M
            with torch.no_grad():
                core(self.zeros("x", M * 512 * 4).view(torch.float32)[:M * 512].view(M // tokens, tokens, 512))
            return
        x3, w3 = self.zeros("x3", lib.avd_split3_bytes(M, K)), self.zeros("w3", lib.avd_split3_bytes(N, K))
        bias = self.zeros("bias", N * 4).view(torch.float32)
        if entry == "qkv3":
            tokens = max(n for n in range(1, 2049) if M % n == 0)
            img = self.zeros("img", lib.avd_qkv3_bytes(M // tokens, tokens, N // 192))
            if terms == 3:
                L.check(lib.avd_gemm_f16x2_qkv_f32(x3.data_ptr(), w3.data_ptr(), bias.data_ptr(), img.data_ptr(), M, tokens, N // 192, K,
                                                   0.18, 1.0, 1.0, st))
            else:
                L.check(lib.avd_gemm_bf16x3_qkv3_f32(x3.data_ptr(), w3.data_ptr(), bias.data_ptr(), img.data_ptr(), M, tokens, N // 192, K,
                                                     0.18, terms, st))
            return
        o = LINEAR[entry]
        r = self.zeros("r", M * N * 4).data_ptr() if o.get("residual") else None
        c = None if o.get("image") else self.zeros("c", M * N * 4).data_ptr()
        c3 = self.zeros("c3", lib.avd_split3_bytes(M, N)).data_ptr() if o.get("image") else None
        act = L.ACT_GELU if o.get("gelu") else L.ACT_NONE
        if terms == 3:
            L.check(lib.avd_gemm_f16x2_f32(x3.data_ptr(), w3.data_ptr(), bias.data_ptr(), r, c, c3, M, N, K, act, 1.0, 1.0, st))
        else:
            L.check(lib.avd_gemm_bf16x3_f32(x3.data_ptr(), w3.data_ptr(), bias.data_ptr(), r, c, c3, M, N, K, act, terms, st))

    def tags(self, case):
        entry, terms, M, N, K, keys = case
        with tuned(**keys):
            self.L.prof_enable(True)
            try:
                self.launch(entry, terms, M, N, K)
                torch.cuda.synchronize()
            finally:
                self.L.prof_enable(False)
        return sorted(k for k, v in self.L.prof_report().items() if v[0] > 0 and (k.startswith("gemm_bf16x3") or k.startswith("splitk_reduce")))


def record(path):
    """writes the table below for the library in the tree (run once on the commit whose choices are to be kept)"""
    run = _Runner(torch.device("cuda:0"))
    table = {_case_id(c): run.tags(c) for c in _cases()}
    kernels = sorted({t for tags in table.values() for t in tags})
    with open(path, "w") as f:
        f.write("KERNELS = [\n" + "".join(f"    {k!r},\n" for k in kernels) + "]\n")
        f.write("EXPECT = {\n" + "".join(f"    {k!r}: {[kernels.index(t) for t in v]},\n" for k, v in table.items()) + "}\n")


@pytest.mark.parametrize("entry", list(LINEAR) + ["qkv3", "core"])
def test_launch_choice_is_the_recorded_one(dev, entry):
    run = _Runner(dev)
    cases = [c for c in _cases() if c[0] == entry]
    assert cases and len({_case_id(c) for c in cases}) == len(cases)
    wrong = {}
    for c in cases:
        got, want = run.tags(c), [KERNELS[i] for i in EXPECT[_case_id(c)]]
        if got != sorted(want):
            wrong[_case_id(c)] = (got, want)
    assert not wrong, wrong


# recorded by record() on the parent of the commit that collapsed the launch ladders; EXPECT values index KERNELS
KERNELS = [
    'gemm_bf16x3_kernel<0, 1, 4>',
    'gemm_bf16x3_kernel<0, 1, 8>',
    'gemm_bf16x3_kernel<0, 3, 4>',
    'gemm_bf16x3_kernel<0, 3, 8>',
    'gemm_bf16x3_kernel<0, 6, 4>',
    'gemm_bf16x3_kernel<0, 6, 8>',
    'gemm_bf16x3_kernel<0, 9, 4>',
    'gemm_bf16x3_kernel<0, 9, 8>',
    'gemm_bf16x3_kernel<2, 1, 4>',
    'gemm_bf16x3_kernel<2, 1, 8>',
    'gemm_bf16x3_kernel<2, 3, 4>',
    'gemm_bf16x3_kernel<2, 3, 8>',
    'gemm_bf16x3_kernel<2, 6, 4>',
    'gemm_bf16x3_kernel<2, 6, 8>',
    'gemm_bf16x3_kernel<2, 9, 4>',
    'gemm_bf16x3_kernel<2, 9, 8>',
    'gemm_bf16x3_kernel<3, 1, 4>',
    'gemm_bf16x3_kernel<3, 3, 4>',
    'gemm_bf16x3_kernel<3, 6, 4>',
    'gemm_bf16x3_kernel<3, 9, 4>',
    'gemm_bf16x3_kernel<4, 1, 4>',
    'gemm_bf16x3_kernel<4, 3, 4>',
    'gemm_bf16x3_kernel<4, 6, 4>',
    'gemm_bf16x3_kernel<4, 9, 4>',
    'gemm_bf16x3_kernel<5, 1, 4>',
    'gemm_bf16x3_kernel<5, 3, 4>',
    'gemm_bf16x3_kernel<5, 6, 4>',
    'gemm_bf16x3_kernel<5, 9, 4>',
    'gemm_bf16x3_kernel<6, 1, 4>',
    'gemm_bf16x3_kernel<6, 1, 8>',
    'gemm_bf16x3_kernel<6, 6, 4>',
    'gemm_bf16x3_kernel<6, 6, 8>',
    'gemm_bf16x3_kernel<6, 9, 4>',
    'gemm_bf16x3_kernel<6, 9, 8>',
    'gemm_bf16x3_kernel<7, 3, 8>',
    'gemm_bf16x3_m16_kernel<0, 4, 8, 0>',
    'gemm_bf16x3_m16_kernel<0, 8, 8, 0>',
    'gemm_bf16x3_m16_kernel<3, 4, 5, 0>',
    'gemm_bf16x3_m16_kernel<3, 4, 6, 0>',
    'gemm_bf16x3_m16_kernel<3, 4, 7, 0>',
    'gemm_bf16x3_m16_kernel<3, 4, 8, 0>',
    'gemm_bf16x3_m16_kernel<3, 8, 8, 0>',
    'gemm_bf16x3_m16_kernel<4, 4, 5, 0>',
    'gemm_bf16x3_m16_kernel<4, 4, 6, 0>',
    'gemm_bf16x3_m16_kernel<4, 4, 7, 0>',
    'gemm_bf16x3_m16_kernel<4, 4, 8, 0>',
    'gemm_bf16x3_m16_kernel<4, 8, 8, 0>',
    'gemm_bf16x3_m16_kernel<5, 4, 2, 4>',
    'gemm_bf16x3_m16_kernel<5, 4, 3, 4>',
    'gemm_bf16x3_m16_kernel<5, 4, 4, 4>',
    'gemm_bf16x3_m16_kernel<5, 4, 5, 4>',
    'gemm_bf16x3_m16_kernel<5, 4, 6, 4>',
    'gemm_bf16x3_m16_kernel<5, 4, 7, 4>',
    'gemm_bf16x3_m16_kernel<5, 4, 8, 0>',
    'gemm_bf16x3_m16_kernel<5, 4, 8, 4>',
    'gemm_bf16x3_m16_kernel<5, 8, 8, 0>',
    'gemm_bf16x3_m16_kernel<6, 4, 2, 0>',
    'gemm_bf16x3_m16_kernel<6, 4, 2, 4>',
    'gemm_bf16x3_m16_kernel<6, 4, 3, 0>',
    'gemm_bf16x3_m16_kernel<6, 4, 3, 4>',
    'gemm_bf16x3_m16_kernel<6, 4, 4, 4>',
    'gemm_bf16x3_m16_kernel<6, 4, 5, 0>',
    'gemm_bf16x3_m16_kernel<6, 4, 5, 4>',
    'gemm_bf16x3_m16_kernel<6, 4, 6, 0>',
    'gemm_bf16x3_m16_kernel<6, 4, 6, 4>',
    'gemm_bf16x3_m16_kernel<6, 4, 7, 4>',
    'gemm_bf16x3_m16_kernel<6, 4, 8, 4>',
    'gemm_bf16x3_m16_kernel<6, 8, 7, 0>',
    'gemm_bf16x3_m16_kernel<8, 4, 2, 4>',
    'gemm_bf16x3_m16_kernel<8, 4, 3, 4>',
    'gemm_bf16x3_m16_kernel<8, 4, 4, 4>',
    'gemm_bf16x3_m16_kernel<8, 4, 5, 4>',
    'gemm_bf16x3_m16_kernel<8, 4, 6, 4>',
    'gemm_bf16x3_m16_kernel<8, 4, 7, 4>',
    'gemm_bf16x3_m16_kernel<8, 4, 8, 4>',
    'gemm_bf16x3_w128_kernel<3, 8>',
    'gemm_bf16x3_w128_kernel<4, 8>',
    'gemm_bf16x3_w128_kernel<5, 8>',
    'gemm_bf16x3_w128_kernel<6, 6>',
    'gemm_bf16x3_w128_kernel<6, 7>',
    'gemm_bf16x3_w128_kernel<6, 8>',
    'splitk_reduce_kernel',
]
EXPECT = {
    'bias t6 M1 N256 K512': [68],
    'bias t6 M300 N256 K512': [68],
    'bias t6 M8192 N256 K512': [68],
    'bias t6 M8193 N256 K512': [69],
    'bias t6 M12288 N256 K512': [69],
    'bias t6 M12289 N256 K512': [70],
    'bias t6 M16384 N256 K512': [70],
    'bias t6 M16385 N256 K512': [71],
    'bias t6 M20480 N256 K512': [71],
    'bias t6 M20481 N256 K512': [72],
    'bias t6 M24576 N256 K512': [72],
    'bias t6 M24577 N256 K512': [73],
    'bias t6 M28672 N256 K512': [73],
    'bias t6 M28673 N256 K512': [74],
    'bias t6 M32768 N256 K512': [74],
    'bias t6 M32769 N256 K512': [35],
    'bias t6 M48896 N256 K512': [35],
    'bias t6 M48897 N256 K512': [36],
    'bias t6 M1 N512 K512': [68],
    'bias t6 M300 N512 K512': [68],
    'bias t6 M4096 N512 K512': [68],
    'bias t6 M4097 N512 K512': [69],
    'bias t6 M6144 N512 K512': [69],
    'bias t6 M6145 N512 K512': [70],
    'bias t6 M8192 N512 K512': [70],
    'bias t6 M8193 N512 K512': [71],
    'bias t6 M10240 N512 K512': [71],
    'bias t6 M10241 N512 K512': [72],
    'bias t6 M12288 N512 K512': [72],
    'bias t6 M12289 N512 K512': [73],
    'bias t6 M14336 N512 K512': [73],
    'bias t6 M14337 N512 K512': [74],
    'bias t6 M16384 N512 K512': [74],
    'bias t6 M16385 N512 K512': [35],
    'bias t6 M24320 N512 K512': [35],
    'bias t6 M24321 N512 K512': [36],
    'bias t6 M300 N512 K512 s3_tile=0': [36],
    'bias t6 M300 N512 K512 s3_tile=1': [68],
    'bias t6 M300 N512 K512 s3_m16=0': [4],
    'bias t6 M300 N512 K512 s3_w128=0': [68],
    'bias t6 M300 N512 K512 s3_rt=7': [68],
    'bias t6 M300 N512 K512 s3_rt=8': [68],
    'bias t6 M300 N512 K512 s3_deep4=0': [35],
    'bias t6 M300 N512 K512 s3_rt=7 s3_tile=0 s3_w128=0': [36],
    'bias t6 M300 N512 K512 s3_rt4=2': [68],
    'bias t6 M300 N512 K512 s3_rt4=3': [69],
    'bias t6 M300 N512 K512 s3_rt4=4': [70],
    'bias t6 M300 N512 K512 s3_rt4=5': [71],
    'bias t6 M300 N512 K512 s3_rt4=6': [72],
    'bias t6 M300 N512 K512 s3_rt4=7': [73],
    'bias t6 M300 N512 K512 s3_rt4=8': [74],
    'bias t9 M300 N512 K512': [6],
    'bias t9 M300 N512 K1024': [6],
    'bias t1 M300 N512 K512': [0],
    'bias t1 M300 N512 K1024': [0],
    'bias t3 M300 N512 K512': [2],
    'bias t3 M300 N512 K1024': [2],
    'bias t6 M300 N512 K1024': [68],
    'bias t6 M4097 N512 K512 s3_tile=0': [36],
    'bias t6 M4097 N512 K512 s3_tile=1': [69],
    'bias t6 M4097 N512 K512 s3_m16=0': [4],
    'bias t6 M4097 N512 K512 s3_w128=0': [69],
    'bias t6 M4097 N512 K512 s3_rt=7': [69],
    'bias t6 M4097 N512 K512 s3_rt=8': [69],
    'bias t6 M4097 N512 K512 s3_deep4=0': [35],
    'bias t6 M4097 N512 K512 s3_rt=7 s3_tile=0 s3_w128=0': [36],
    'bias t6 M4097 N512 K512 s3_rt4=2': [35],
    'bias t6 M4097 N512 K512 s3_rt4=3': [69],
    'bias t6 M4097 N512 K512 s3_rt4=4': [70],
    'bias t6 M4097 N512 K512 s3_rt4=5': [71],
    'bias t6 M4097 N512 K512 s3_rt4=6': [72],
    'bias t6 M4097 N512 K512 s3_rt4=7': [73],
    'bias t6 M4097 N512 K512 s3_rt4=8': [74],
    'bias t9 M4097 N512 K512': [6],
    'bias t9 M4097 N512 K1024': [6],
    'bias t1 M4097 N512 K512': [0],
    'bias t1 M4097 N512 K1024': [0],
    'bias t3 M4097 N512 K512': [2],
    'bias t3 M4097 N512 K1024': [2],
    'bias t6 M4097 N512 K1024': [69],
    'bias t6 M24321 N512 K512 s3_tile=0': [36],
    'bias t6 M24321 N512 K512 s3_tile=1': [35],
    'bias t6 M24321 N512 K512 s3_m16=0': [5],
    'bias t6 M24321 N512 K512 s3_w128=0': [36],
    'bias t6 M24321 N512 K512 s3_rt=7': [36],
    'bias t6 M24321 N512 K512 s3_rt=8': [36],
    'bias t6 M24321 N512 K512 s3_deep4=0': [36],
    'bias t6 M24321 N512 K512 s3_rt=7 s3_tile=0 s3_w128=0': [36],
    'bias t6 M24321 N512 K512 s3_rt4=2': [36],
    'bias t6 M24321 N512 K512 s3_rt4=3': [36],
    'bias t6 M24321 N512 K512 s3_rt4=4': [36],
    'bias t6 M24321 N512 K512 s3_rt4=5': [36],
    'bias t6 M24321 N512 K512 s3_rt4=6': [36],
    'bias t6 M24321 N512 K512 s3_rt4=7': [36],
    'bias t6 M24321 N512 K512 s3_rt4=8': [36],
    'bias t9 M24321 N512 K512': [7],
    'bias t9 M24321 N512 K1024': [7],
    'bias t1 M24321 N512 K512': [1],
    'bias t1 M24321 N512 K1024': [1],
    'bias t3 M24321 N512 K512': [3],
    'bias t3 M24321 N512 K1024': [3],
    'bias t6 M24321 N512 K1024': [36],
    'residual t6 M1 N256 K512': [57],
    'residual t6 M300 N256 K512': [57],
    'residual t6 M8192 N256 K512': [57],
    'residual t6 M8193 N256 K512': [59],
    'residual t6 M12288 N256 K512': [59],
    'residual t6 M12289 N256 K512': [60],
    'residual t6 M16384 N256 K512': [60],
    'residual t6 M16385 N256 K512': [62],
    'residual t6 M20480 N256 K512': [62],
    'residual t6 M20481 N256 K512': [64],
    'residual t6 M24576 N256 K512': [64],
    'residual t6 M24577 N256 K512': [65],
    'residual t6 M28672 N256 K512': [65],
    'residual t6 M28673 N256 K512': [66],
    'residual t6 M32768 N256 K512': [66],
    'residual t6 M32769 N256 K512': [61],
    'residual t6 M48896 N256 K512': [63],
    'residual t6 M48897 N256 K512': [78],
    'residual t6 M49152 N256 K512': [78],
    'residual t6 M49153 N256 K512': [79],
    'residual t6 M57344 N256 K512': [79],
    'residual t6 M57345 N256 K512': [80],
    'residual t6 M1 N512 K512': [57],
    'residual t6 M300 N512 K512': [57],
    'residual t6 M4096 N512 K512': [57],
    'residual t6 M4097 N512 K512': [59],
    'residual t6 M6144 N512 K512': [59],
    'residual t6 M6145 N512 K512': [60],
    'residual t6 M8192 N512 K512': [60],
    'residual t6 M8193 N512 K512': [62],
    'residual t6 M10240 N512 K512': [62],
    'residual t6 M10241 N512 K512': [64],
    'residual t6 M12288 N512 K512': [64],
    'residual t6 M12289 N512 K512': [65],
    'residual t6 M14336 N512 K512': [65],
    'residual t6 M14337 N512 K512': [66],
    'residual t6 M16384 N512 K512': [66],
    'residual t6 M16385 N512 K512': [61],
    'residual t6 M24320 N512 K512': [63],
    'residual t6 M24321 N512 K512': [78],
    'residual t6 M24576 N512 K512': [78],
    'residual t6 M24577 N512 K512': [79],
    'residual t6 M28672 N512 K512': [79],
    'residual t6 M28673 N512 K512': [80],
    'residual t6 M32768 N512 K512': [80],
    'residual t6 M32769 N512 K512': [78],
    'residual t6 M300 N512 K512 s3_tile=0': [78],
    'residual t6 M300 N512 K512 s3_tile=1': [57],
    'residual t6 M300 N512 K512 s3_m16=0': [12],
    'residual t6 M300 N512 K512 s3_w128=0': [57],
    'residual t6 M300 N512 K512 s3_rt=7': [57],
    'residual t6 M300 N512 K512 s3_rt=8': [57],
    'residual t6 M300 N512 K512 s3_deep4=0': [56],
    'residual t6 M300 N512 K512 s3_rt=7 s3_tile=0 s3_w128=0': [67],
    'residual t6 M300 N512 K512 s3_rt4=2': [57],
    'residual t6 M300 N512 K512 s3_rt4=3': [59],
    'residual t6 M300 N512 K512 s3_rt4=4': [60],
    'residual t6 M300 N512 K512 s3_rt4=5': [62],
    'residual t6 M300 N512 K512 s3_rt4=6': [64],
    'residual t6 M300 N512 K512 s3_rt4=7': [65],
    'residual t6 M300 N512 K512 s3_rt4=8': [66],
    'residual t9 M300 N512 K512': [14],
    'residual t9 M300 N512 K1024': [14],
    'residual t1 M300 N512 K512': [8],
    'residual t1 M300 N512 K1024': [8],
    'residual t3 M300 N512 K512': [10],
    'residual t3 M300 N512 K1024': [10],
    'residual t6 M300 N512 K1024': [57],
    'residual t6 M4097 N512 K512 s3_tile=0': [78],
    'residual t6 M4097 N512 K512 s3_tile=1': [59],
    'residual t6 M4097 N512 K512 s3_m16=0': [12],
    'residual t6 M4097 N512 K512 s3_w128=0': [59],
    'residual t6 M4097 N512 K512 s3_rt=7': [59],
    'residual t6 M4097 N512 K512 s3_rt=8': [59],
    'residual t6 M4097 N512 K512 s3_deep4=0': [58],
    'residual t6 M4097 N512 K512 s3_rt=7 s3_tile=0 s3_w128=0': [67],
    'residual t6 M4097 N512 K512 s3_rt4=2': [56],
    'residual t6 M4097 N512 K512 s3_rt4=3': [59],
    'residual t6 M4097 N512 K512 s3_rt4=4': [60],
    'residual t6 M4097 N512 K512 s3_rt4=5': [62],
    'residual t6 M4097 N512 K512 s3_rt4=6': [64],
    'residual t6 M4097 N512 K512 s3_rt4=7': [65],
    'residual t6 M4097 N512 K512 s3_rt4=8': [66],
    'residual t9 M4097 N512 K512': [14],
    'residual t9 M4097 N512 K1024': [14],
    'residual t1 M4097 N512 K512': [8],
    'residual t1 M4097 N512 K1024': [8],
    'residual t3 M4097 N512 K512': [10],
    'residual t3 M4097 N512 K1024': [10],
    'residual t6 M4097 N512 K1024': [59],
    'residual t6 M24321 N512 K512 s3_tile=0': [78],
    'residual t6 M24321 N512 K512 s3_tile=1': [63],
    'residual t6 M24321 N512 K512 s3_m16=0': [13],
    'residual t6 M24321 N512 K512 s3_w128=0': [67],
    'residual t6 M24321 N512 K512 s3_rt=7': [79],
    'residual t6 M24321 N512 K512 s3_rt=8': [80],
    'residual t6 M24321 N512 K512 s3_deep4=0': [78],
    'residual t6 M24321 N512 K512 s3_rt=7 s3_tile=0 s3_w128=0': [67],
    'residual t6 M24321 N512 K512 s3_rt4=2': [78],
    'residual t6 M24321 N512 K512 s3_rt4=3': [78],
    'residual t6 M24321 N512 K512 s3_rt4=4': [78],
    'residual t6 M24321 N512 K512 s3_rt4=5': [78],
    'residual t6 M24321 N512 K512 s3_rt4=6': [78],
    'residual t6 M24321 N512 K512 s3_rt4=7': [78],
    'residual t6 M24321 N512 K512 s3_rt4=8': [78],
    'residual t9 M24321 N512 K512': [15],
    'residual t9 M24321 N512 K1024': [15],
    'residual t1 M24321 N512 K512': [9],
    'residual t1 M24321 N512 K1024': [9],
    'residual t3 M24321 N512 K512': [11],
    'residual t3 M24321 N512 K1024': [11],
    'residual t6 M24321 N512 K1024': [78],
    'gelu_image t6 M1 N256 K512': [37],
    'gelu_image t6 M300 N256 K512': [37],
    'gelu_image t6 M8192 N256 K512': [37],
    'gelu_image t6 M8193 N256 K512': [37],
    'gelu_image t6 M12288 N256 K512': [37],
    'gelu_image t6 M12289 N256 K512': [37],
    'gelu_image t6 M16384 N256 K512': [37],
    'gelu_image t6 M16385 N256 K512': [37],
    'gelu_image t6 M20480 N256 K512': [37],
    'gelu_image t6 M20481 N256 K512': [38],
    'gelu_image t6 M24576 N256 K512': [38],
    'gelu_image t6 M24577 N256 K512': [39],
    'gelu_image t6 M28672 N256 K512': [39],
    'gelu_image t6 M28673 N256 K512': [40],
    'gelu_image t6 M32768 N256 K512': [40],
    'gelu_image t6 M32769 N256 K512': [37],
    'gelu_image t6 M40960 N256 K512': [37],
    'gelu_image t6 M40961 N256 K512': [38],
    'gelu_image t6 M48896 N256 K512': [38],
    'gelu_image t6 M48897 N256 K512': [38],
    'gelu_image t6 M1 N512 K512': [37],
    'gelu_image t6 M300 N512 K512': [37],
    'gelu_image t6 M4096 N512 K512': [37],
    'gelu_image t6 M4097 N512 K512': [37],
    'gelu_image t6 M6144 N512 K512': [37],
    'gelu_image t6 M6145 N512 K512': [37],
    'gelu_image t6 M8192 N512 K512': [37],
    'gelu_image t6 M8193 N512 K512': [37],
    'gelu_image t6 M10240 N512 K512': [37],
    'gelu_image t6 M10241 N512 K512': [38],
    'gelu_image t6 M12288 N512 K512': [38],
    'gelu_image t6 M12289 N512 K512': [39],
    'gelu_image t6 M14336 N512 K512': [39],
    'gelu_image t6 M14337 N512 K512': [40],
    'gelu_image t6 M16384 N512 K512': [40],
    'gelu_image t6 M16385 N512 K512': [37],
    'gelu_image t6 M20480 N512 K512': [37],
    'gelu_image t6 M20481 N512 K512': [38],
    'gelu_image t6 M24320 N512 K512': [38],
    'gelu_image t6 M24321 N512 K512': [38],
    'gelu_image t6 M1 N2048 K512': [37],
    'gelu_image t6 M300 N2048 K512': [37],
    'gelu_image t6 M1024 N2048 K512': [37],
    'gelu_image t6 M1025 N2048 K512': [37],
    'gelu_image t6 M1536 N2048 K512': [37],
    'gelu_image t6 M1537 N2048 K512': [37],
    'gelu_image t6 M2048 N2048 K512': [37],
    'gelu_image t6 M2049 N2048 K512': [37],
    'gelu_image t6 M2560 N2048 K512': [37],
    'gelu_image t6 M2561 N2048 K512': [38],
    'gelu_image t6 M3072 N2048 K512': [38],
    'gelu_image t6 M3073 N2048 K512': [39],
    'gelu_image t6 M3584 N2048 K512': [39],
    'gelu_image t6 M3585 N2048 K512': [40],
    'gelu_image t6 M4096 N2048 K512': [40],
    'gelu_image t6 M4097 N2048 K512': [37],
    'gelu_image t6 M5120 N2048 K512': [37],
    'gelu_image t6 M5121 N2048 K512': [38],
    'gelu_image t6 M5888 N2048 K512': [38],
    'gelu_image t6 M5889 N2048 K512': [38],
    'gelu_image t6 M300 N512 K512 s3_tile=0': [75],
    'gelu_image t6 M300 N512 K512 s3_tile=1': [37],
    'gelu_image t6 M300 N512 K512 s3_m16=0': [18],
    'gelu_image t6 M300 N512 K512 s3_w128=0': [37],
    'gelu_image t6 M300 N512 K512 s3_rt=7': [37],
    'gelu_image t6 M300 N512 K512 s3_rt=8': [37],
    'gelu_image t6 M300 N512 K512 s3_deep4=0': [37],
    'gelu_image t6 M300 N512 K512 s3_rt=7 s3_tile=0 s3_w128=0': [41],
    'gelu_image t6 M300 N512 K512 s3_rt4=2': [37],
    'gelu_image t6 M300 N512 K512 s3_rt4=3': [37],
    'gelu_image t6 M300 N512 K512 s3_rt4=4': [37],
    'gelu_image t6 M300 N512 K512 s3_rt4=5': [37],
    'gelu_image t6 M300 N512 K512 s3_rt4=6': [38],
    'gelu_image t6 M300 N512 K512 s3_rt4=7': [39],
    'gelu_image t6 M300 N512 K512 s3_rt4=8': [40],
    'gelu_image t9 M300 N512 K512': [19],
    'gelu_image t9 M300 N512 K1024': [19],
    'gelu_image t1 M300 N512 K512': [16],
    'gelu_image t1 M300 N512 K1024': [16],
    'gelu_image t3 M300 N512 K512': [17],
    'gelu_image t3 M300 N512 K1024': [17],
    'gelu_image t6 M300 N512 K1024': [37],
    'gelu_image t6 M4097 N512 K512 s3_tile=0': [75],
    'gelu_image t6 M4097 N512 K512 s3_tile=1': [37],
    'gelu_image t6 M4097 N512 K512 s3_m16=0': [18],
    'gelu_image t6 M4097 N512 K512 s3_w128=0': [37],
    'gelu_image t6 M4097 N512 K512 s3_rt=7': [37],
    'gelu_image t6 M4097 N512 K512 s3_rt=8': [37],
    'gelu_image t6 M4097 N512 K512 s3_deep4=0': [37],
    'gelu_image t6 M4097 N512 K512 s3_rt=7 s3_tile=0 s3_w128=0': [41],
    'gelu_image t6 M4097 N512 K512 s3_rt4=2': [37],
    'gelu_image t6 M4097 N512 K512 s3_rt4=3': [37],
    'gelu_image t6 M4097 N512 K512 s3_rt4=4': [37],
    'gelu_image t6 M4097 N512 K512 s3_rt4=5': [37],
    'gelu_image t6 M4097 N512 K512 s3_rt4=6': [38],
    'gelu_image t6 M4097 N512 K512 s3_rt4=7': [39],
    'gelu_image t6 M4097 N512 K512 s3_rt4=8': [40],
    'gelu_image t9 M4097 N512 K512': [19],
    'gelu_image t9 M4097 N512 K1024': [19],
    'gelu_image t1 M4097 N512 K512': [16],
    'gelu_image t1 M4097 N512 K1024': [16],
    'gelu_image t3 M4097 N512 K512': [17],
    'gelu_image t3 M4097 N512 K1024': [17],
    'gelu_image t6 M4097 N512 K1024': [37],
    'gelu_image t6 M24321 N512 K512 s3_tile=0': [75],
    'gelu_image t6 M24321 N512 K512 s3_tile=1': [38],
    'gelu_image t6 M24321 N512 K512 s3_m16=0': [18],
    'gelu_image t6 M24321 N512 K512 s3_w128=0': [38],
    'gelu_image t6 M24321 N512 K512 s3_rt=7': [38],
    'gelu_image t6 M24321 N512 K512 s3_rt=8': [38],
    'gelu_image t6 M24321 N512 K512 s3_deep4=0': [38],
    'gelu_image t6 M24321 N512 K512 s3_rt=7 s3_tile=0 s3_w128=0': [41],
    'gelu_image t6 M24321 N512 K512 s3_rt4=2': [37],
    'gelu_image t6 M24321 N512 K512 s3_rt4=3': [37],
    'gelu_image t6 M24321 N512 K512 s3_rt4=4': [37],
    'gelu_image t6 M24321 N512 K512 s3_rt4=5': [37],
    'gelu_image t6 M24321 N512 K512 s3_rt4=6': [38],
    'gelu_image t6 M24321 N512 K512 s3_rt4=7': [39],
    'gelu_image t6 M24321 N512 K512 s3_rt4=8': [40],
    'gelu_image t9 M24321 N512 K512': [19],
    'gelu_image t9 M24321 N512 K1024': [19],
    'gelu_image t1 M24321 N512 K512': [16],
    'gelu_image t1 M24321 N512 K1024': [16],
    'gelu_image t3 M24321 N512 K512': [17],
    'gelu_image t3 M24321 N512 K1024': [17],
    'gelu_image t6 M24321 N512 K1024': [38],
    'image t6 M1 N256 K512': [47],
    'image t6 M300 N256 K512': [47],
    'image t6 M8192 N256 K512': [47],
    'image t6 M8193 N256 K512': [48],
    'image t6 M12288 N256 K512': [48],
    'image t6 M12289 N256 K512': [49],
    'image t6 M16384 N256 K512': [49],
    'image t6 M16385 N256 K512': [50],
    'image t6 M20480 N256 K512': [50],
    'image t6 M20481 N256 K512': [51],
    'image t6 M24576 N256 K512': [51],
    'image t6 M24577 N256 K512': [52],
    'image t6 M28672 N256 K512': [52],
    'image t6 M28673 N256 K512': [54],
    'image t6 M32768 N256 K512': [54],
    'image t6 M32769 N256 K512': [53],
    'image t6 M48896 N256 K512': [53],
    'image t6 M48897 N256 K512': [53],
    'image t6 M1 N512 K512': [47],
    'image t6 M300 N512 K512': [47],
    'image t6 M4096 N512 K512': [47],
    'image t6 M4097 N512 K512': [48],
    'image t6 M6144 N512 K512': [48],
    'image t6 M6145 N512 K512': [49],
    'image t6 M8192 N512 K512': [49],
    'image t6 M8193 N512 K512': [50],
    'image t6 M10240 N512 K512': [50],
    'image t6 M10241 N512 K512': [51],
    'image t6 M12288 N512 K512': [51],
    'image t6 M12289 N512 K512': [52],
    'image t6 M14336 N512 K512': [52],
    'image t6 M14337 N512 K512': [54],
    'image t6 M16384 N512 K512': [54],
    'image t6 M16385 N512 K512': [53],
    'image t6 M24320 N512 K512': [53],
    'image t6 M24321 N512 K512': [53],
    'image t6 M300 N512 K512 s3_tile=0': [77],
    'image t6 M300 N512 K512 s3_tile=1': [47],
    'image t6 M300 N512 K512 s3_m16=0': [26],
    'image t6 M300 N512 K512 s3_w128=0': [47],
    'image t6 M300 N512 K512 s3_rt=7': [47],
    'image t6 M300 N512 K512 s3_rt=8': [47],
    'image t6 M300 N512 K512 s3_deep4=0': [53],
    'image t6 M300 N512 K512 s3_rt=7 s3_tile=0 s3_w128=0': [55],
    'image t6 M300 N512 K512 s3_rt4=2': [47],
    'image t6 M300 N512 K512 s3_rt4=3': [48],
    'image t6 M300 N512 K512 s3_rt4=4': [49],
    'image t6 M300 N512 K512 s3_rt4=5': [50],
    'image t6 M300 N512 K512 s3_rt4=6': [51],
    'image t6 M300 N512 K512 s3_rt4=7': [52],
    'image t6 M300 N512 K512 s3_rt4=8': [54],
    'image t9 M300 N512 K512': [27],
    'image t9 M300 N512 K1024': [27],
    'image t1 M300 N512 K512': [24],
    'image t1 M300 N512 K1024': [24],
    'image t3 M300 N512 K512': [25],
    'image t3 M300 N512 K1024': [25],
    'image t6 M300 N512 K1024': [47],
    'image t6 M4097 N512 K512 s3_tile=0': [77],
    'image t6 M4097 N512 K512 s3_tile=1': [48],
    'image t6 M4097 N512 K512 s3_m16=0': [26],
    'image t6 M4097 N512 K512 s3_w128=0': [48],
    'image t6 M4097 N512 K512 s3_rt=7': [48],
    'image t6 M4097 N512 K512 s3_rt=8': [48],
    'image t6 M4097 N512 K512 s3_deep4=0': [53],
    'image t6 M4097 N512 K512 s3_rt=7 s3_tile=0 s3_w128=0': [55],
    'image t6 M4097 N512 K512 s3_rt4=2': [53],
    'image t6 M4097 N512 K512 s3_rt4=3': [48],
    'image t6 M4097 N512 K512 s3_rt4=4': [49],
    'image t6 M4097 N512 K512 s3_rt4=5': [50],
    'image t6 M4097 N512 K512 s3_rt4=6': [51],
    'image t6 M4097 N512 K512 s3_rt4=7': [52],
    'image t6 M4097 N512 K512 s3_rt4=8': [54],
    'image t9 M4097 N512 K512': [27],
    'image t9 M4097 N512 K1024': [27],
    'image t1 M4097 N512 K512': [24],
    'image t1 M4097 N512 K1024': [24],
    'image t3 M4097 N512 K512': [25],
    'image t3 M4097 N512 K1024': [25],
    'image t6 M4097 N512 K1024': [48],
    'image t6 M24321 N512 K512 s3_tile=0': [77],
    'image t6 M24321 N512 K512 s3_tile=1': [53],
    'image t6 M24321 N512 K512 s3_m16=0': [26],
    'image t6 M24321 N512 K512 s3_w128=0': [53],
    'image t6 M24321 N512 K512 s3_rt=7': [53],
    'image t6 M24321 N512 K512 s3_rt=8': [53],
    'image t6 M24321 N512 K512 s3_deep4=0': [53],
    'image t6 M24321 N512 K512 s3_rt=7 s3_tile=0 s3_w128=0': [55],
    'image t6 M24321 N512 K512 s3_rt4=2': [53],
    'image t6 M24321 N512 K512 s3_rt4=3': [53],
    'image t6 M24321 N512 K512 s3_rt4=4': [53],
    'image t6 M24321 N512 K512 s3_rt4=5': [53],
    'image t6 M24321 N512 K512 s3_rt4=6': [53],
    'image t6 M24321 N512 K512 s3_rt4=7': [53],
    'image t6 M24321 N512 K512 s3_rt4=8': [53],
    'image t9 M24321 N512 K512': [27],
    'image t9 M24321 N512 K1024': [27],
    'image t1 M24321 N512 K512': [24],
    'image t1 M24321 N512 K1024': [24],
    'image t3 M24321 N512 K512': [25],
    'image t3 M24321 N512 K1024': [25],
    'image t6 M24321 N512 K1024': [53],
    'qkv3 t6 M1 N1536 K512': [42],
    'qkv3 t6 M300 N1536 K512': [42],
    'qkv3 t6 M1344 N1536 K512': [42],
    'qkv3 t6 M1345 N1536 K512': [42],
    'qkv3 t6 M2016 N1536 K512': [42],
    'qkv3 t6 M2017 N1536 K512': [42],
    'qkv3 t6 M2688 N1536 K512': [42],
    'qkv3 t6 M2689 N1536 K512': [42],
    'qkv3 t6 M3360 N1536 K512': [42],
    'qkv3 t6 M3361 N1536 K512': [43],
    'qkv3 t6 M4032 N1536 K512': [43],
    'qkv3 t6 M4033 N1536 K512': [44],
    'qkv3 t6 M4704 N1536 K512': [44],
    'qkv3 t6 M4705 N1536 K512': [45],
    'qkv3 t6 M5376 N1536 K512': [45],
    'qkv3 t6 M5377 N1536 K512': [42],
    'qkv3 t6 M6720 N1536 K512': [42],
    'qkv3 t6 M6721 N1536 K512': [43],
    'qkv3 t6 M7936 N1536 K512': [43],
    'qkv3 t6 M7937 N1536 K512': [43],
    'qkv3 t6 M300 N1536 K512 s3_tile=0': [76],
    'qkv3 t6 M300 N1536 K512 s3_tile=1': [42],
    'qkv3 t6 M300 N1536 K512 s3_m16=0': [22],
    'qkv3 t6 M300 N1536 K512 s3_w128=0': [42],
    'qkv3 t6 M300 N1536 K512 s3_rt=7': [42],
    'qkv3 t6 M300 N1536 K512 s3_rt=8': [42],
    'qkv3 t6 M300 N1536 K512 s3_deep4=0': [42],
    'qkv3 t6 M300 N1536 K512 s3_rt=7 s3_tile=0 s3_w128=0': [46],
    'qkv3 t6 M300 N1536 K512 s3_rt4=2': [42],
    'qkv3 t6 M300 N1536 K512 s3_rt4=3': [42],
    'qkv3 t6 M300 N1536 K512 s3_rt4=4': [42],
    'qkv3 t6 M300 N1536 K512 s3_rt4=5': [42],
    'qkv3 t6 M300 N1536 K512 s3_rt4=6': [43],
    'qkv3 t6 M300 N1536 K512 s3_rt4=7': [44],
    'qkv3 t6 M300 N1536 K512 s3_rt4=8': [45],
    'qkv3 t9 M300 N1536 K512': [23],
    'qkv3 t9 M300 N1536 K1024': [23],
    'qkv3 t1 M300 N1536 K512': [20],
    'qkv3 t1 M300 N1536 K1024': [20],
    'qkv3 t3 M300 N1536 K512': [21],
    'qkv3 t3 M300 N1536 K1024': [21],
    'qkv3 t6 M4097 N1536 K512 s3_tile=0': [76],
    'qkv3 t6 M4097 N1536 K512 s3_tile=1': [44],
    'qkv3 t6 M4097 N1536 K512 s3_m16=0': [22],
    'qkv3 t6 M4097 N1536 K512 s3_w128=0': [44],
    'qkv3 t6 M4097 N1536 K512 s3_rt=7': [44],
    'qkv3 t6 M4097 N1536 K512 s3_rt=8': [44],
    'qkv3 t6 M4097 N1536 K512 s3_deep4=0': [44],
    'qkv3 t6 M4097 N1536 K512 s3_rt=7 s3_tile=0 s3_w128=0': [46],
    'qkv3 t6 M4097 N1536 K512 s3_rt4=2': [42],
    'qkv3 t6 M4097 N1536 K512 s3_rt4=3': [42],
    'qkv3 t6 M4097 N1536 K512 s3_rt4=4': [42],
    'qkv3 t6 M4097 N1536 K512 s3_rt4=5': [42],
    'qkv3 t6 M4097 N1536 K512 s3_rt4=6': [43],
    'qkv3 t6 M4097 N1536 K512 s3_rt4=7': [44],
    'qkv3 t6 M4097 N1536 K512 s3_rt4=8': [45],
    'qkv3 t9 M4097 N1536 K512': [23],
    'qkv3 t9 M4097 N1536 K1024': [23],
    'qkv3 t1 M4097 N1536 K512': [20],
    'qkv3 t1 M4097 N1536 K1024': [20],
    'qkv3 t3 M4097 N1536 K512': [21],
    'qkv3 t3 M4097 N1536 K1024': [21],
    'qkv3 t6 M24321 N1536 K512 s3_tile=0': [76],
    'qkv3 t6 M24321 N1536 K512 s3_tile=1': [45],
    'qkv3 t6 M24321 N1536 K512 s3_m16=0': [22],
    'qkv3 t6 M24321 N1536 K512 s3_w128=0': [45],
    'qkv3 t6 M24321 N1536 K512 s3_rt=7': [45],
    'qkv3 t6 M24321 N1536 K512 s3_rt=8': [45],
    'qkv3 t6 M24321 N1536 K512 s3_deep4=0': [45],
    'qkv3 t6 M24321 N1536 K512 s3_rt=7 s3_tile=0 s3_w128=0': [46],
    'qkv3 t6 M24321 N1536 K512 s3_rt4=2': [42],
    'qkv3 t6 M24321 N1536 K512 s3_rt4=3': [42],
    'qkv3 t6 M24321 N1536 K512 s3_rt4=4': [42],
    'qkv3 t6 M24321 N1536 K512 s3_rt4=5': [42],
    'qkv3 t6 M24321 N1536 K512 s3_rt4=6': [43],
    'qkv3 t6 M24321 N1536 K512 s3_rt4=7': [44],
    'qkv3 t6 M24321 N1536 K512 s3_rt4=8': [45],
    'qkv3 t9 M24321 N1536 K512': [23],
    'qkv3 t9 M24321 N1536 K1024': [23],
    'qkv3 t1 M24321 N1536 K512': [20],
    'qkv3 t1 M24321 N1536 K1024': [20],
    'qkv3 t3 M24321 N1536 K512': [21],
    'qkv3 t3 M24321 N1536 K1024': [21],
    'core t6 M300 N512 K1024 s3_min_rows=0': [37, 42, 57],
    'core t6 M4096 N512 K1024 s3_min_rows=0': [37, 44, 57],
    'core t6 M4097 N512 K1024 s3_min_rows=0': [37, 44, 59],
    'core t6 M8192 N512 K1024 s3_min_rows=0': [40, 44, 60],
    'core t6 M8193 N512 K1024 s3_min_rows=0': [37, 44, 62],
    'core t6 M24320 N512 K1024 s3_min_rows=0': [40, 45, 63],
    'core t6 M24321 N512 K1024 s3_min_rows=0': [40, 45, 78],
    'core t6 M4097 N512 K1024 s3_min_rows=0 s3_splitk=0': [37, 44, 59],
    'core t6 M4097 N512 K1024 s3_min_rows=0 s3_splitk=2': [37, 44, 59],
    'core t6 M4097 N512 K1024 s3_min_rows=0 s3_tile=0': [75, 76, 78],
    'core t6 M4097 N512 K1024 s3_min_rows=0 s3_tile=1': [37, 44, 59],
    'core t6 M4097 N512 K1024 s3_m16=0 s3_min_rows=0': [4, 18, 22, 30, 81],
    'core t6 M4097 N512 K1024 s3_min_rows=0 s3_w128=0': [37, 44, 59],
    'core t6 M4097 N512 K1024 s3_min_rows=0 s3_rt=7': [37, 44, 59],
    'core t6 M4097 N512 K1024 s3_min_rows=0 s3_rt=8': [37, 44, 59],
    'core t6 M4097 N512 K1024 s3_deep4=0 s3_min_rows=0': [37, 44, 58],
    'core t6 M4097 N512 K1024 s3_min_rows=0 s3_rt=7 s3_tile=0 s3_w128=0': [41, 46, 67],
    'core t6 M4097 N512 K1024 s3_min_rows=0 s3_rt4=2': [37, 42, 56],
    'core t6 M4097 N512 K1024 s3_min_rows=0 s3_rt4=3': [37, 42, 59],
    'core t6 M4097 N512 K1024 s3_min_rows=0 s3_rt4=4': [37, 42, 60],
    'core t6 M4097 N512 K1024 s3_min_rows=0 s3_rt4=5': [37, 42, 62],
    'core t6 M4097 N512 K1024 s3_min_rows=0 s3_rt4=6': [38, 43, 64],
    'core t6 M4097 N512 K1024 s3_min_rows=0 s3_rt4=7': [39, 44, 65],
    'core t6 M4097 N512 K1024 s3_min_rows=0 s3_rt4=8': [40, 45, 66],
    'core t6 M24321 N512 K1024 s3_min_rows=0 s3_splitk=0': [40, 45, 78],
    'core t6 M24321 N512 K1024 s3_min_rows=0 s3_splitk=2': [40, 45, 78],
    'core t6 M24321 N512 K1024 s3_min_rows=0 s3_tile=0': [75, 76, 78],
    'core t6 M24321 N512 K1024 s3_min_rows=0 s3_tile=1': [40, 45, 63],
    'core t6 M24321 N512 K1024 s3_m16=0 s3_min_rows=0': [13, 18, 22, 31],
    'core t6 M24321 N512 K1024 s3_min_rows=0 s3_w128=0': [40, 45, 67],
    'core t6 M24321 N512 K1024 s3_min_rows=0 s3_rt=7': [40, 45, 79],
    'core t6 M24321 N512 K1024 s3_min_rows=0 s3_rt=8': [40, 45, 80],
    'core t6 M24321 N512 K1024 s3_deep4=0 s3_min_rows=0': [40, 45, 78],
    'core t6 M24321 N512 K1024 s3_min_rows=0 s3_rt=7 s3_tile=0 s3_w128=0': [41, 46, 67],
    'core t6 M24321 N512 K1024 s3_min_rows=0 s3_rt4=2': [37, 42, 78],
    'core t6 M24321 N512 K1024 s3_min_rows=0 s3_rt4=3': [37, 42, 78],
    'core t6 M24321 N512 K1024 s3_min_rows=0 s3_rt4=4': [37, 42, 78],
    'core t6 M24321 N512 K1024 s3_min_rows=0 s3_rt4=5': [37, 42, 78],
    'core t6 M24321 N512 K1024 s3_min_rows=0 s3_rt4=6': [38, 43, 78],
    'core t6 M24321 N512 K1024 s3_min_rows=0 s3_rt4=7': [39, 44, 78],
    'core t6 M24321 N512 K1024 s3_min_rows=0 s3_rt4=8': [40, 45, 78],
    'core t6 M1 N512 K2048 s3_min_rows=0': [37, 42, 57],
    'core t6 M300 N512 K2048 s3_min_rows=0': [37, 42, 57],
    'core t6 M4096 N512 K2048 s3_min_rows=0': [40, 44, 57],
    'core t6 M4097 N512 K2048 s3_min_rows=0': [37, 44, 59],
    'core t6 M6144 N512 K2048 s3_min_rows=0': [38, 42, 59],
    'core t6 M6145 N512 K2048 s3_min_rows=0': [39, 42, 60],
    'core t6 M8192 N512 K2048 s3_min_rows=0': [40, 44, 60],
    'core t6 M8193 N512 K2048 s3_min_rows=0': [38, 44, 62],
    'core t6 M10240 N512 K2048 s3_min_rows=0': [39, 45, 62],
    'core t6 M10241 N512 K2048 s3_min_rows=0': [39, 45, 64],
    'core t6 M12288 N512 K2048 s3_min_rows=0': [40, 43, 64],
    'core t6 M12289 N512 K2048 s3_min_rows=0': [39, 44, 65],
    'core t6 M14336 N512 K2048 s3_min_rows=0': [39, 44, 65],
    'core t6 M14337 N512 K2048 s3_min_rows=0': [40, 45, 66],
    'core t6 M16384 N512 K2048 s3_min_rows=0': [40, 45, 66],
    'core t6 M16385 N512 K2048 s3_min_rows=0': [39, 44, 61],
    'core t6 M24320 N512 K2048 s3_min_rows=0': [40, 45, 63],
    'core t6 M24321 N512 K2048 s3_min_rows=0': [40, 45, 78],
    'core t6 M24576 N512 K2048 s3_min_rows=0': [40, 45, 78],
    'core t6 M24577 N512 K2048 s3_min_rows=0': [39, 45, 79],
    'core t6 M28672 N512 K2048 s3_min_rows=0': [40, 44, 79],
    'core t6 M28673 N512 K2048 s3_min_rows=0': [40, 45, 80],
    'core t6 M32768 N512 K2048 s3_min_rows=0': [40, 45, 80],
    'core t6 M32769 N512 K2048 s3_min_rows=0': [40, 44, 78],
    'core t6 M4097 N512 K2048 s3_min_rows=0 s3_splitk=0': [37, 44, 59],
    'core t6 M4097 N512 K2048 s3_min_rows=0 s3_splitk=2': [37, 44, 59],
    'core t6 M4097 N512 K2048 s3_min_rows=0 s3_tile=0': [75, 76, 78],
    'core t6 M4097 N512 K2048 s3_min_rows=0 s3_tile=1': [37, 44, 59],
    'core t6 M4097 N512 K2048 s3_m16=0 s3_min_rows=0': [4, 18, 22, 30, 81],
    'core t6 M4097 N512 K2048 s3_min_rows=0 s3_w128=0': [37, 44, 59],
    'core t6 M4097 N512 K2048 s3_min_rows=0 s3_rt=7': [37, 44, 59],
    'core t6 M4097 N512 K2048 s3_min_rows=0 s3_rt=8': [37, 44, 59],
    'core t6 M4097 N512 K2048 s3_deep4=0 s3_min_rows=0': [37, 44, 58],
    'core t6 M4097 N512 K2048 s3_min_rows=0 s3_rt=7 s3_tile=0 s3_w128=0': [41, 46, 67],
    'core t6 M4097 N512 K2048 s3_min_rows=0 s3_rt4=2': [37, 42, 56],
    'core t6 M4097 N512 K2048 s3_min_rows=0 s3_rt4=3': [37, 42, 59],
    'core t6 M4097 N512 K2048 s3_min_rows=0 s3_rt4=4': [37, 42, 60],
    'core t6 M4097 N512 K2048 s3_min_rows=0 s3_rt4=5': [37, 42, 62],
    'core t6 M4097 N512 K2048 s3_min_rows=0 s3_rt4=6': [38, 43, 64],
    'core t6 M4097 N512 K2048 s3_min_rows=0 s3_rt4=7': [39, 44, 65],
    'core t6 M4097 N512 K2048 s3_min_rows=0 s3_rt4=8': [40, 45, 66],
    'core t6 M24321 N512 K2048 s3_min_rows=0 s3_splitk=0': [40, 45, 78],
    'core t6 M24321 N512 K2048 s3_min_rows=0 s3_splitk=2': [40, 45, 78],
    'core t6 M24321 N512 K2048 s3_min_rows=0 s3_tile=0': [75, 76, 78],
    'core t6 M24321 N512 K2048 s3_min_rows=0 s3_tile=1': [40, 45, 63],
    'core t6 M24321 N512 K2048 s3_m16=0 s3_min_rows=0': [13, 18, 22, 31],
    'core t6 M24321 N512 K2048 s3_min_rows=0 s3_w128=0': [40, 45, 67],
    'core t6 M24321 N512 K2048 s3_min_rows=0 s3_rt=7': [40, 45, 79],
    'core t6 M24321 N512 K2048 s3_min_rows=0 s3_rt=8': [40, 45, 80],
    'core t6 M24321 N512 K2048 s3_deep4=0 s3_min_rows=0': [40, 45, 78],
    'core t6 M24321 N512 K2048 s3_min_rows=0 s3_rt=7 s3_tile=0 s3_w128=0': [41, 46, 67],
    'core t6 M24321 N512 K2048 s3_min_rows=0 s3_rt4=2': [37, 42, 78],
    'core t6 M24321 N512 K2048 s3_min_rows=0 s3_rt4=3': [37, 42, 78],
    'core t6 M24321 N512 K2048 s3_min_rows=0 s3_rt4=4': [37, 42, 78],
    'core t6 M24321 N512 K2048 s3_min_rows=0 s3_rt4=5': [37, 42, 78],
    'core t6 M24321 N512 K2048 s3_min_rows=0 s3_rt4=6': [38, 43, 78],
    'core t6 M24321 N512 K2048 s3_min_rows=0 s3_rt4=7': [39, 44, 78],
    'core t6 M24321 N512 K2048 s3_min_rows=0 s3_rt4=8': [40, 45, 78],
    'core t9 M300 N512 K1024 s3_min_rows=0': [6, 19, 23, 32, 81],
    'core t9 M4096 N512 K1024 s3_min_rows=0': [6, 19, 23, 32, 81],
    'core t9 M4097 N512 K1024 s3_min_rows=0': [6, 19, 23, 32, 81],
    'core t9 M8192 N512 K1024 s3_min_rows=0': [6, 19, 23, 32, 81],
    'core t9 M8193 N512 K1024 s3_min_rows=0': [14, 19, 23, 32],
    'core t9 M24320 N512 K1024 s3_min_rows=0': [14, 19, 23, 32],
    'core t9 M24321 N512 K1024 s3_min_rows=0': [15, 19, 23, 33],
    'core t9 M4097 N512 K1024 s3_min_rows=0 s3_splitk=0': [14, 19, 23, 32],
    'core t9 M4097 N512 K1024 s3_min_rows=0 s3_splitk=2': [6, 19, 23, 32, 81],
    'core t9 M24321 N512 K1024 s3_min_rows=0 s3_splitk=0': [15, 19, 23, 33],
    'core t9 M24321 N512 K1024 s3_min_rows=0 s3_splitk=2': [15, 19, 23, 33],
    'core t9 M300 N512 K2048 s3_min_rows=0': [6, 19, 23, 32, 81],
    'core t9 M4096 N512 K2048 s3_min_rows=0': [6, 19, 23, 32, 81],
    'core t9 M4097 N512 K2048 s3_min_rows=0': [6, 19, 23, 32, 81],
    'core t9 M8192 N512 K2048 s3_min_rows=0': [6, 19, 23, 32, 81],
    'core t9 M8193 N512 K2048 s3_min_rows=0': [14, 19, 23, 32],
    'core t9 M24320 N512 K2048 s3_min_rows=0': [14, 19, 23, 32],
    'core t9 M24321 N512 K2048 s3_min_rows=0': [15, 19, 23, 33],
    'core t9 M4097 N512 K2048 s3_min_rows=0 s3_splitk=0': [14, 19, 23, 32],
    'core t9 M4097 N512 K2048 s3_min_rows=0 s3_splitk=2': [6, 19, 23, 32, 81],
    'core t9 M24321 N512 K2048 s3_min_rows=0 s3_splitk=0': [15, 19, 23, 33],
    'core t9 M24321 N512 K2048 s3_min_rows=0 s3_splitk=2': [15, 19, 23, 33],
    'core t1 M300 N512 K1024 s3_min_rows=0': [0, 16, 20, 28, 81],
    'core t1 M4096 N512 K1024 s3_min_rows=0': [0, 16, 20, 28, 81],
    'core t1 M4097 N512 K1024 s3_min_rows=0': [0, 16, 20, 28, 81],
    'core t1 M8192 N512 K1024 s3_min_rows=0': [0, 16, 20, 28, 81],
    'core t1 M8193 N512 K1024 s3_min_rows=0': [8, 16, 20, 28],
    'core t1 M24320 N512 K1024 s3_min_rows=0': [8, 16, 20, 28],
    'core t1 M24321 N512 K1024 s3_min_rows=0': [9, 16, 20, 29],
    'core t1 M4097 N512 K1024 s3_min_rows=0 s3_splitk=0': [8, 16, 20, 28],
    'core t1 M4097 N512 K1024 s3_min_rows=0 s3_splitk=2': [0, 16, 20, 28, 81],
    'core t1 M24321 N512 K1024 s3_min_rows=0 s3_splitk=0': [9, 16, 20, 29],
    'core t1 M24321 N512 K1024 s3_min_rows=0 s3_splitk=2': [9, 16, 20, 29],
    'core t1 M300 N512 K2048 s3_min_rows=0': [0, 16, 20, 28, 81],
    'core t1 M4096 N512 K2048 s3_min_rows=0': [0, 16, 20, 28, 81],
    'core t1 M4097 N512 K2048 s3_min_rows=0': [0, 16, 20, 28, 81],
    'core t1 M8192 N512 K2048 s3_min_rows=0': [0, 16, 20, 28, 81],
    'core t1 M8193 N512 K2048 s3_min_rows=0': [8, 16, 20, 28],
    'core t1 M24320 N512 K2048 s3_min_rows=0': [8, 16, 20, 28],
    'core t1 M24321 N512 K2048 s3_min_rows=0': [9, 16, 20, 29],
    'core t1 M4097 N512 K2048 s3_min_rows=0 s3_splitk=0': [8, 16, 20, 28],
    'core t1 M4097 N512 K2048 s3_min_rows=0 s3_splitk=2': [0, 16, 20, 28, 81],
    'core t1 M24321 N512 K2048 s3_min_rows=0 s3_splitk=0': [9, 16, 20, 29],
    'core t1 M24321 N512 K2048 s3_min_rows=0 s3_splitk=2': [9, 16, 20, 29],
    'core t3 M300 N512 K1024 s3_min_rows=0': [10, 17, 21, 34],
    'core t3 M4096 N512 K1024 s3_min_rows=0': [10, 17, 21, 34],
    'core t3 M4097 N512 K1024 s3_min_rows=0': [10, 17, 21, 34],
    'core t3 M8192 N512 K1024 s3_min_rows=0': [10, 17, 21, 34],
    'core t3 M8193 N512 K1024 s3_min_rows=0': [10, 17, 21, 34],
    'core t3 M24320 N512 K1024 s3_min_rows=0': [10, 17, 21, 34],
    'core t3 M24321 N512 K1024 s3_min_rows=0': [11, 17, 21, 34],
    'core t3 M4097 N512 K1024 s3_min_rows=0 s3_splitk=0': [10, 17, 21, 34],
    'core t3 M4097 N512 K1024 s3_min_rows=0 s3_splitk=2': [10, 17, 21, 34],
    'core t3 M24321 N512 K1024 s3_min_rows=0 s3_splitk=0': [11, 17, 21, 34],
    'core t3 M24321 N512 K1024 s3_min_rows=0 s3_splitk=2': [11, 17, 21, 34],
    'core t3 M300 N512 K2048 s3_min_rows=0': [10, 17, 21, 34],
    'core t3 M4096 N512 K2048 s3_min_rows=0': [10, 17, 21, 34],
    'core t3 M4097 N512 K2048 s3_min_rows=0': [10, 17, 21, 34],
    'core t3 M8192 N512 K2048 s3_min_rows=0': [10, 17, 21, 34],
    'core t3 M8193 N512 K2048 s3_min_rows=0': [10, 17, 21, 34],
    'core t3 M24320 N512 K2048 s3_min_rows=0': [10, 17, 21, 34],
    'core t3 M24321 N512 K2048 s3_min_rows=0': [11, 17, 21, 34],
    'core t3 M4097 N512 K2048 s3_min_rows=0 s3_splitk=0': [10, 17, 21, 34],
    'core t3 M4097 N512 K2048 s3_min_rows=0 s3_splitk=2': [10, 17, 21, 34],
    'core t3 M24321 N512 K2048 s3_min_rows=0 s3_splitk=0': [11, 17, 21, 34],
    'core t3 M24321 N512 K2048 s3_min_rows=0 s3_splitk=2': [11, 17, 21, 34],
}
