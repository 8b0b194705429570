"""Which kernels the VideoVAE host code picks (csrc/vae3d_f32.hip: the decode and encode routes and the conv launch), pinned through
the profiling tags.  Every case is one VideoVAE.decode or .encode call on a tiny input whose tiles are ragged; EXPECT holds the
(tag, launches, work) triples each case ran, recorded on a5c3b51, the commit before the conv launch ladder and the two route bodies were
collapsed.  Launches are compared exactly and the work to 1e-9 relative (products of integers and one 14 / 27 factor).  Outputs are not
checked here (tests/test_gpu_vae_outputs.py compares every case of this file with the fp64 oracle)."""
import pytest
import torch

from _tune import tuned

pytestmark = pytest.mark.gpu

MODES = ("f32", "bf16x3", "f16x2")
# decode: latent [2, Cv, 2, 3, 5] -> (8, 24, 40) (W ragged for the 4 x (4 | 8) x 16 halo tile) and -> (6, 18, 40) (T, H, W ragged for
# both tile heights; 4,320 voxels is no multiple of the fp32 kernel's 128)
DEC_OUT = {"8x24x40": None, "6x18x40": (6, 18, 40)}
# encode: (input T, H, W), (t_down, s_down); pooling (2, 4, 4) has no partial-sums kernel and must take gn_pool_tolat_kernel
ENC_IN = {"pool488": ((8, 16, 24), (4, 8)), "pool244": ((6, 12, 20), (2, 4))}


def _decode_cases():
    """(mode, dec_blocks, Cv, lat_composed, lat_packed, vae_fold, vae_lat, shape), without the combinations a mode ignores: "f32" reads
    none of the four switches; the Python side composes the first conv for Cv <= 16 only and packs its taps for Cv <= 8 only"""
    out = []
    for shape in DEC_OUT:
        for nb in (1, 2, 3):
            for cv in (8, 12, 24):
                out.append(("f32", nb, cv, False, False, 1, 1, shape))
                lat = [(False, False)] + ([(True, False)] if cv <= 16 else []) + ([(True, True)] if cv <= 8 else [])
                out += [(mode, nb, cv, lc, lp, fold, 1, shape) for mode in MODES[1:] for lc, lp in lat for fold in (0, 1)]
    out += [(mode, 2, 8, True, True, 1, 0, "8x24x40") for mode in MODES]          # "vae_lat" 0: one row per mode
    return [("decode",) + c for c in out]


def _encode_cases():
    """(mode, enc_blocks, enc_packed, vae_fold, shape): the 4 -> 64 first conv is fp32 in every mode, so one block reads no switch;
    enc_packed is read by "bf16x3" with two blocks only"""
    out = []
    for shape in ENC_IN:
        for nb in (1, 2, 3):
            out.append(("f32", nb, False, 1, shape))
            for mode in MODES[1:]:
                packed = (False, True) if mode == "bf16x3" and nb == 2 else (False,)
                out += [(mode, nb, pk, fold, shape) for pk in packed for fold in ((0, 1) if nb > 1 else (1,))]
    return [("encode",) + c for c in out]


def _cases():
    return _decode_cases() + _encode_cases()


def _case_id(case):
    if case[0] == "decode":
        _, mode, nb, cv, lc, lp, fold, lat, shape = case
        return f"decode {mode} blocks{nb} Cv{cv} composed{int(lc)} packed{int(lp)} fold{fold} lat{lat} {shape}"
    _, mode, nb, pk, fold, shape = case
    return f"encode {mode} blocks{nb} packed{int(pk)} fold{fold} {shape}"


class _Runner:
    """runs one case: call(case) is the plain VideoVAE call, triples(case) its sorted (tag, launches, work) with launches > 0"""

    def __init__(self, dev):
        from multimodal_diffusion_amd import _lib as L
        self.dev, self.L = dev, L
        self.vaes, self.inputs = {}, {}

    def vae(self, nb, cv, t_down, s_down):
        import multimodal_diffusion_amd as A
        key = (nb, cv, t_down, s_down)
        if key not in self.vaes:
            torch.manual_seed(1000 * nb + 10 * cv + t_down)
            cfg = A.VideoVAEConfig(lat_ch=cv, t_down=t_down, s_down=s_down, enc_blocks=nb, dec_blocks=nb)
            self.vaes[key] = A.VideoVAE(cfg).to(self.dev).eval()
        return self.vaes[key]

    def input(self, *shape):
        if shape not in self.inputs:
            g = torch.Generator().manual_seed(sum(shape))
            self.inputs[shape] = torch.randn(*shape, generator=g).to(self.dev)
        return self.inputs[shape]

    def prepare(self, case):
        """-> (the VideoVAE of the case with its switches set, the call, the tune keys)"""
        if case[0] == "decode":
            _, mode, nb, cv, lc, lp, fold, lat, shape = case
            vae = self.vae(nb, cv, 4, 8)
            vae.matmul, vae.lat_composed, vae.lat_packed = mode, lc, lp
            z = self.input(2, cv, 2, 3, 5)
            return vae, (lambda: vae.decode(z, out_size=DEC_OUT[shape])), dict(vae_fold=fold, vae_lat=lat)
        _, mode, nb, pk, fold, shape = case
        (T, H, W), (td, sd) = ENC_IN[shape]
        vae = self.vae(nb, 8, td, sd)
        vae.matmul, vae.enc_packed = mode, pk
        x = self.input(2, 3, T, H, W)
        return vae, (lambda: vae.encode(x)), dict(vae_fold=fold)

    def triples(self, case):
        _, call, keys = self.prepare(case)
        with tuned(**keys):
            call()              # the weight images and their scales are cached here, outside the recorded call
            self.L.prof_enable(True)
            try:
                call()
                torch.cuda.synchronize()
            finally:
                self.L.prof_enable(False)
        return sorted((k, v[0], v[2]) for k, v in self.L.prof_report().items() if v[0] > 0)


def record(path):
    """writes the table below for the library in the tree (run once on the commit whose choices are to be kept)"""
    run = _Runner(torch.device("cuda:0"))
    table = {_case_id(c): run.triples(c) for c in _cases()}
    kernels = sorted({t[0] for v in table.values() for t in v})
    with open(path, "w") as f:
        f.write("KERNELS = [\n" + "".join(f"    {k!r},\n" for k in kernels) + "]\n")
        f.write("EXPECT = {\n" + "".join(f"    {k!r}: {[(kernels.index(t), n, w) for t, n, w in v]},\n" for k, v in table.items()) + "}\n")


@pytest.fixture(scope="module")
def runner():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return _Runner(torch.device("cuda:0"))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("direction", ["decode", "encode"])
def test_route_is_the_recorded_one(runner, direction, mode):
    cases = [c for c in _cases() if c[0] == direction and c[1] == mode]
    assert cases and len({_case_id(c) for c in cases}) == len(cases)
    wrong = {}
    for c in cases:
        got, want = runner.triples(c), sorted((KERNELS[i], n, w) for i, n, w in EXPECT[_case_id(c)])
        same = len(got) == len(want) and all(g[:2] == w[:2] and abs(g[2] - w[2]) <= 1e-9 * abs(w[2]) for g, w in zip(got, want))
        if not same:
            wrong[_case_id(c)] = (got, want)
    assert not wrong, wrong


def test_every_case_is_recorded():
    assert sorted(EXPECT) == sorted(_case_id(c) for c in _cases())


# recorded by record() on a5c3b51; EXPECT values are (index into KERNELS, launches, work)
KERNELS = [
    'conv3_weight_gn_kernel',
    'conv3d_k3_bf16x3_kernel<3, 0, 0>',
    'conv3d_k3_bf16x3_kernel<3, 1, 0>',
    'conv3d_k3_bf16x3_kernel<3, 4, 0>',
    'conv3d_k3_bf16x3_kernel<3, 4, 2>',
    'conv3d_k3_bf16x3_kernel<3, 4, 3>',
    'conv3d_k3_bf16x3_kernel<6, 0, 0>',
    'conv3d_k3_bf16x3_kernel<6, 0, 1>',
    'conv3d_k3_bf16x3_kernel<6, 1, 0>',
    'conv3d_k3_bf16x3_kernel<6, 1, 1>',
    'conv3d_k3_bf16x3_kernel<6, 4, 0>',
    'conv3d_k3_bf16x3_kernel<6, 4, 2>',
    'conv3d_k3_bf16x3_kernel<6, 4, 3>',
    'conv3d_k3_gelu_stats_kernel<4>',
    'conv3d_k3_gelu_stats_kernel<64>',
    'fromlat_kernel',
    'gn_apply_pad3_kernel',
    'gn_apply_pad_kernel',
    'gn_apply_toimg_kernel',
    'gn_pool_tolat_kernel',
    'pool_tolat_from_partials_kernel',
    'rgb_lat16_kernel',
    'toimg_from_p_kernel',
    'upsample_lat16_kernel',
    'upsample_lat8_kernel',
    'upsample_pad3_kernel',
    'upsample_pad_kernel',
]
EXPECT = {
    'decode f32 blocks1 Cv8 composed0 packed0 fold1 lat1 8x24x40': [(14, 1, 3397386240.0), (15, 1, 17280.0), (18, 1, 4116480.0), (26, 1, 3932160.0)],
    'decode bf16x3 blocks1 Cv8 composed0 packed0 fold0 lat1 8x24x40': [(10, 1, 3397386240.0), (15, 1, 17280.0), (18, 1, 4116480.0), (25, 1, 5898240.0)],
    'decode bf16x3 blocks1 Cv8 composed0 packed0 fold1 lat1 8x24x40': [(11, 1, 3397386240.0), (15, 1, 17280.0), (22, 1, 2150400.0), (25, 1, 5898240.0)],
    'decode bf16x3 blocks1 Cv8 composed1 packed0 fold0 lat1 8x24x40': [(8, 1, 849346560.0), (18, 1, 4116480.0), (24, 1, 1474560.0)],
    'decode bf16x3 blocks1 Cv8 composed1 packed0 fold1 lat1 8x24x40': [(8, 1, 849346560.0), (18, 1, 4116480.0), (24, 1, 1474560.0)],
    'decode bf16x3 blocks1 Cv8 composed1 packed1 fold0 lat1 8x24x40': [(6, 1, 440401920.0), (18, 1, 4116480.0), (24, 1, 1474560.0)],
    'decode bf16x3 blocks1 Cv8 composed1 packed1 fold1 lat1 8x24x40': [(6, 1, 440401920.0), (18, 1, 4116480.0), (24, 1, 1474560.0)],
    'decode f16x2 blocks1 Cv8 composed0 packed0 fold0 lat1 8x24x40': [(3, 1, 3397386240.0), (15, 1, 17280.0), (18, 1, 4116480.0), (25, 1, 5898240.0)],
    'decode f16x2 blocks1 Cv8 composed0 packed0 fold1 lat1 8x24x40': [(4, 1, 3397386240.0), (15, 1, 17280.0), (22, 1, 2150400.0), (25, 1, 5898240.0)],
    'decode f16x2 blocks1 Cv8 composed1 packed0 fold0 lat1 8x24x40': [(2, 1, 849346560.0), (18, 1, 4116480.0), (24, 1, 1474560.0)],
    'decode f16x2 blocks1 Cv8 composed1 packed0 fold1 lat1 8x24x40': [(2, 1, 849346560.0), (18, 1, 4116480.0), (24, 1, 1474560.0)],
    'decode f16x2 blocks1 Cv8 composed1 packed1 fold0 lat1 8x24x40': [(1, 1, 440401920.0), (18, 1, 4116480.0), (24, 1, 1474560.0)],
    'decode f16x2 blocks1 Cv8 composed1 packed1 fold1 lat1 8x24x40': [(1, 1, 440401920.0), (18, 1, 4116480.0), (24, 1, 1474560.0)],
    'decode f32 blocks1 Cv12 composed0 packed0 fold1 lat1 8x24x40': [(14, 1, 3397386240.0), (15, 1, 18240.0), (18, 1, 4116480.0), (26, 1, 3932160.0)],
    'decode bf16x3 blocks1 Cv12 composed0 packed0 fold0 lat1 8x24x40': [(10, 1, 3397386240.0), (15, 1, 18240.0), (18, 1, 4116480.0), (25, 1, 5898240.0)],
    'decode bf16x3 blocks1 Cv12 composed0 packed0 fold1 lat1 8x24x40': [(11, 1, 3397386240.0), (15, 1, 18240.0), (22, 1, 2150400.0), (25, 1, 5898240.0)],
    'decode bf16x3 blocks1 Cv12 composed1 packed0 fold0 lat1 8x24x40': [(8, 1, 849346560.0), (18, 1, 4116480.0), (23, 1, 1474560.0)],
    'decode bf16x3 blocks1 Cv12 composed1 packed0 fold1 lat1 8x24x40': [(8, 1, 849346560.0), (18, 1, 4116480.0), (23, 1, 1474560.0)],
    'decode f16x2 blocks1 Cv12 composed0 packed0 fold0 lat1 8x24x40': [(3, 1, 3397386240.0), (15, 1, 18240.0), (18, 1, 4116480.0), (25, 1, 5898240.0)],
    'decode f16x2 blocks1 Cv12 composed0 packed0 fold1 lat1 8x24x40': [(4, 1, 3397386240.0), (15, 1, 18240.0), (22, 1, 2150400.0), (25, 1, 5898240.0)],
    'decode f16x2 blocks1 Cv12 composed1 packed0 fold0 lat1 8x24x40': [(2, 1, 849346560.0), (18, 1, 4116480.0), (23, 1, 1474560.0)],
    'decode f16x2 blocks1 Cv12 composed1 packed0 fold1 lat1 8x24x40': [(2, 1, 849346560.0), (18, 1, 4116480.0), (23, 1, 1474560.0)],
    'decode f32 blocks1 Cv24 composed0 packed0 fold1 lat1 8x24x40': [(14, 1, 3397386240.0), (15, 1, 21120.0), (18, 1, 4116480.0), (26, 1, 3932160.0)],
    'decode bf16x3 blocks1 Cv24 composed0 packed0 fold0 lat1 8x24x40': [(10, 1, 3397386240.0), (15, 1, 21120.0), (18, 1, 4116480.0), (25, 1, 5898240.0)],
    'decode bf16x3 blocks1 Cv24 composed0 packed0 fold1 lat1 8x24x40': [(11, 1, 3397386240.0), (15, 1, 21120.0), (22, 1, 2150400.0), (25, 1, 5898240.0)],
    'decode f16x2 blocks1 Cv24 composed0 packed0 fold0 lat1 8x24x40': [(3, 1, 3397386240.0), (15, 1, 21120.0), (18, 1, 4116480.0), (25, 1, 5898240.0)],
    'decode f16x2 blocks1 Cv24 composed0 packed0 fold1 lat1 8x24x40': [(4, 1, 3397386240.0), (15, 1, 21120.0), (22, 1, 2150400.0), (25, 1, 5898240.0)],
    'decode f32 blocks2 Cv8 composed0 packed0 fold1 lat1 8x24x40': [(14, 2, 6794772480.0), (15, 1, 17280.0), (17, 1, 7864320.0), (18, 1, 4116480.0), (26, 1, 3932160.0)],
    'decode bf16x3 blocks2 Cv8 composed0 packed0 fold0 lat1 8x24x40': [(10, 2, 6794772480.0), (15, 1, 17280.0), (16, 1, 9830400.0), (18, 1, 4116480.0), (25, 1, 5898240.0)],
    'decode bf16x3 blocks2 Cv8 composed0 packed0 fold1 lat1 8x24x40': [(10, 1, 3397386240.0), (11, 1, 3397386240.0), (15, 1, 17280.0), (16, 1, 9830400.0), (22, 1, 2150400.0), (25, 1, 5898240.0)],
    'decode bf16x3 blocks2 Cv8 composed1 packed0 fold0 lat1 8x24x40': [(8, 1, 849346560.0), (10, 1, 3397386240.0), (16, 1, 9830400.0), (18, 1, 4116480.0), (24, 1, 1474560.0)],
    'decode bf16x3 blocks2 Cv8 composed1 packed0 fold1 lat1 8x24x40': [(0, 1, 2211840.0), (9, 1, 849346560.0), (11, 1, 3397386240.0), (22, 1, 2150400.0), (24, 1, 1474560.0)],
    'decode bf16x3 blocks2 Cv8 composed1 packed1 fold0 lat1 8x24x40': [(6, 1, 440401920.0), (10, 1, 3397386240.0), (16, 1, 9830400.0), (18, 1, 4116480.0), (24, 1, 1474560.0)],
    'decode bf16x3 blocks2 Cv8 composed1 packed1 fold1 lat1 8x24x40': [(0, 1, 2211840.0), (7, 1, 440401920.0), (11, 1, 3397386240.0), (22, 1, 2150400.0), (24, 1, 1474560.0)],
    'decode f16x2 blocks2 Cv8 composed0 packed0 fold0 lat1 8x24x40': [(3, 2, 6794772480.0), (15, 1, 17280.0), (16, 1, 9830400.0), (18, 1, 4116480.0), (25, 1, 5898240.0)],
    'decode f16x2 blocks2 Cv8 composed0 packed0 fold1 lat1 8x24x40': [(3, 1, 3397386240.0), (4, 1, 3397386240.0), (15, 1, 17280.0), (16, 1, 9830400.0), (22, 1, 2150400.0), (25, 1, 5898240.0)],
    'decode f16x2 blocks2 Cv8 composed1 packed0 fold0 lat1 8x24x40': [(2, 1, 849346560.0), (3, 1, 3397386240.0), (16, 1, 9830400.0), (18, 1, 4116480.0), (24, 1, 1474560.0)],
    'decode f16x2 blocks2 Cv8 composed1 packed0 fold1 lat1 8x24x40': [(2, 1, 849346560.0), (4, 1, 3397386240.0), (16, 1, 9830400.0), (22, 1, 2150400.0), (24, 1, 1474560.0)],
    'decode f16x2 blocks2 Cv8 composed1 packed1 fold0 lat1 8x24x40': [(1, 1, 440401920.0), (3, 1, 3397386240.0), (16, 1, 9830400.0), (18, 1, 4116480.0), (24, 1, 1474560.0)],
    'decode f16x2 blocks2 Cv8 composed1 packed1 fold1 lat1 8x24x40': [(1, 1, 440401920.0), (4, 1, 3397386240.0), (16, 1, 9830400.0), (22, 1, 2150400.0), (24, 1, 1474560.0)],
    'decode f32 blocks2 Cv12 composed0 packed0 fold1 lat1 8x24x40': [(14, 2, 6794772480.0), (15, 1, 18240.0), (17, 1, 7864320.0), (18, 1, 4116480.0), (26, 1, 3932160.0)],
    'decode bf16x3 blocks2 Cv12 composed0 packed0 fold0 lat1 8x24x40': [(10, 2, 6794772480.0), (15, 1, 18240.0), (16, 1, 9830400.0), (18, 1, 4116480.0), (25, 1, 5898240.0)],
    'decode bf16x3 blocks2 Cv12 composed0 packed0 fold1 lat1 8x24x40': [(10, 1, 3397386240.0), (11, 1, 3397386240.0), (15, 1, 18240.0), (16, 1, 9830400.0), (22, 1, 2150400.0), (25, 1, 5898240.0)],
    'decode bf16x3 blocks2 Cv12 composed1 packed0 fold0 lat1 8x24x40': [(8, 1, 849346560.0), (10, 1, 3397386240.0), (16, 1, 9830400.0), (18, 1, 4116480.0), (23, 1, 1474560.0)],
    'decode bf16x3 blocks2 Cv12 composed1 packed0 fold1 lat1 8x24x40': [(0, 1, 2211840.0), (9, 1, 849346560.0), (11, 1, 3397386240.0), (22, 1, 2150400.0), (23, 1, 1474560.0)],
    'decode f16x2 blocks2 Cv12 composed0 packed0 fold0 lat1 8x24x40': [(3, 2, 6794772480.0), (15, 1, 18240.0), (16, 1, 9830400.0), (18, 1, 4116480.0), (25, 1, 5898240.0)],
    'decode f16x2 blocks2 Cv12 composed0 packed0 fold1 lat1 8x24x40': [(3, 1, 3397386240.0), (4, 1, 3397386240.0), (15, 1, 18240.0), (16, 1, 9830400.0), (22, 1, 2150400.0), (25, 1, 5898240.0)],
    'decode f16x2 blocks2 Cv12 composed1 packed0 fold0 lat1 8x24x40': [(2, 1, 849346560.0), (3, 1, 3397386240.0), (16, 1, 9830400.0), (18, 1, 4116480.0), (23, 1, 1474560.0)],
    'decode f16x2 blocks2 Cv12 composed1 packed0 fold1 lat1 8x24x40': [(2, 1, 849346560.0), (4, 1, 3397386240.0), (16, 1, 9830400.0), (22, 1, 2150400.0), (23, 1, 1474560.0)],
    'decode f32 blocks2 Cv24 composed0 packed0 fold1 lat1 8x24x40': [(14, 2, 6794772480.0), (15, 1, 21120.0), (17, 1, 7864320.0), (18, 1, 4116480.0), (26, 1, 3932160.0)],
    'decode bf16x3 blocks2 Cv24 composed0 packed0 fold0 lat1 8x24x40': [(10, 2, 6794772480.0), (15, 1, 21120.0), (16, 1, 9830400.0), (18, 1, 4116480.0), (25, 1, 5898240.0)],
    'decode bf16x3 blocks2 Cv24 composed0 packed0 fold1 lat1 8x24x40': [(10, 1, 3397386240.0), (11, 1, 3397386240.0), (15, 1, 21120.0), (16, 1, 9830400.0), (22, 1, 2150400.0), (25, 1, 5898240.0)],
    'decode f16x2 blocks2 Cv24 composed0 packed0 fold0 lat1 8x24x40': [(3, 2, 6794772480.0), (15, 1, 21120.0), (16, 1, 9830400.0), (18, 1, 4116480.0), (25, 1, 5898240.0)],
    'decode f16x2 blocks2 Cv24 composed0 packed0 fold1 lat1 8x24x40': [(3, 1, 3397386240.0), (4, 1, 3397386240.0), (15, 1, 21120.0), (16, 1, 9830400.0), (22, 1, 2150400.0), (25, 1, 5898240.0)],
    'decode f32 blocks3 Cv8 composed0 packed0 fold1 lat1 8x24x40': [(14, 3, 10192158720.0), (15, 1, 17280.0), (17, 2, 15728640.0), (18, 1, 4116480.0), (26, 1, 3932160.0)],
    'decode bf16x3 blocks3 Cv8 composed0 packed0 fold0 lat1 8x24x40': [(10, 3, 10192158720.0), (15, 1, 17280.0), (16, 2, 19660800.0), (18, 1, 4116480.0), (25, 1, 5898240.0)],
    'decode bf16x3 blocks3 Cv8 composed0 packed0 fold1 lat1 8x24x40': [(10, 2, 6794772480.0), (11, 1, 3397386240.0), (15, 1, 17280.0), (16, 2, 19660800.0), (22, 1, 2150400.0), (25, 1, 5898240.0)],
    'decode bf16x3 blocks3 Cv8 composed1 packed0 fold0 lat1 8x24x40': [(8, 1, 849346560.0), (10, 2, 6794772480.0), (16, 2, 19660800.0), (18, 1, 4116480.0), (24, 1, 1474560.0)],
    'decode bf16x3 blocks3 Cv8 composed1 packed0 fold1 lat1 8x24x40': [(8, 1, 849346560.0), (10, 1, 3397386240.0), (11, 1, 3397386240.0), (16, 2, 19660800.0), (22, 1, 2150400.0), (24, 1, 1474560.0)],
    'decode bf16x3 blocks3 Cv8 composed1 packed1 fold0 lat1 8x24x40': [(6, 1, 440401920.0), (10, 2, 6794772480.0), (16, 2, 19660800.0), (18, 1, 4116480.0), (24, 1, 1474560.0)],
    'decode bf16x3 blocks3 Cv8 composed1 packed1 fold1 lat1 8x24x40': [(6, 1, 440401920.0), (10, 1, 3397386240.0), (11, 1, 3397386240.0), (16, 2, 19660800.0), (22, 1, 2150400.0), (24, 1, 1474560.0)],
    'decode f16x2 blocks3 Cv8 composed0 packed0 fold0 lat1 8x24x40': [(3, 3, 10192158720.0), (15, 1, 17280.0), (16, 2, 19660800.0), (18, 1, 4116480.0), (25, 1, 5898240.0)],
    'decode f16x2 blocks3 Cv8 composed0 packed0 fold1 lat1 8x24x40': [(3, 2, 6794772480.0), (4, 1, 3397386240.0), (15, 1, 17280.0), (16, 2, 19660800.0), (22, 1, 2150400.0), (25, 1, 5898240.0)],
    'decode f16x2 blocks3 Cv8 composed1 packed0 fold0 lat1 8x24x40': [(2, 1, 849346560.0), (3, 2, 6794772480.0), (16, 2, 19660800.0), (18, 1, 4116480.0), (24, 1, 1474560.0)],
    'decode f16x2 blocks3 Cv8 composed1 packed0 fold1 lat1 8x24x40': [(2, 1, 849346560.0), (3, 1, 3397386240.0), (4, 1, 3397386240.0), (16, 2, 19660800.0), (22, 1, 2150400.0), (24, 1, 1474560.0)],
    'decode f16x2 blocks3 Cv8 composed1 packed1 fold0 lat1 8x24x40': [(1, 1, 440401920.0), (3, 2, 6794772480.0), (16, 2, 19660800.0), (18, 1, 4116480.0), (24, 1, 1474560.0)],
    'decode f16x2 blocks3 Cv8 composed1 packed1 fold1 lat1 8x24x40': [(1, 1, 440401920.0), (3, 1, 3397386240.0), (4, 1, 3397386240.0), (16, 2, 19660800.0), (22, 1, 2150400.0), (24, 1, 1474560.0)],
    'decode f32 blocks3 Cv12 composed0 packed0 fold1 lat1 8x24x40': [(14, 3, 10192158720.0), (15, 1, 18240.0), (17, 2, 15728640.0), (18, 1, 4116480.0), (26, 1, 3932160.0)],
    'decode bf16x3 blocks3 Cv12 composed0 packed0 fold0 lat1 8x24x40': [(10, 3, 10192158720.0), (15, 1, 18240.0), (16, 2, 19660800.0), (18, 1, 4116480.0), (25, 1, 5898240.0)],
    'decode bf16x3 blocks3 Cv12 composed0 packed0 fold1 lat1 8x24x40': [(10, 2, 6794772480.0), (11, 1, 3397386240.0), (15, 1, 18240.0), (16, 2, 19660800.0), (22, 1, 2150400.0), (25, 1, 5898240.0)],
    'decode bf16x3 blocks3 Cv12 composed1 packed0 fold0 lat1 8x24x40': [(8, 1, 849346560.0), (10, 2, 6794772480.0), (16, 2, 19660800.0), (18, 1, 4116480.0), (23, 1, 1474560.0)],
    'decode bf16x3 blocks3 Cv12 composed1 packed0 fold1 lat1 8x24x40': [(8, 1, 849346560.0), (10, 1, 3397386240.0), (11, 1, 3397386240.0), (16, 2, 19660800.0), (22, 1, 2150400.0), (23, 1, 1474560.0)],
    'decode f16x2 blocks3 Cv12 composed0 packed0 fold0 lat1 8x24x40': [(3, 3, 10192158720.0), (15, 1, 18240.0), (16, 2, 19660800.0), (18, 1, 4116480.0), (25, 1, 5898240.0)],
    'decode f16x2 blocks3 Cv12 composed0 packed0 fold1 lat1 8x24x40': [(3, 2, 6794772480.0), (4, 1, 3397386240.0), (15, 1, 18240.0), (16, 2, 19660800.0), (22, 1, 2150400.0), (25, 1, 5898240.0)],
    'decode f16x2 blocks3 Cv12 composed1 packed0 fold0 lat1 8x24x40': [(2, 1, 849346560.0), (3, 2, 6794772480.0), (16, 2, 19660800.0), (18, 1, 4116480.0), (23, 1, 1474560.0)],
    'decode f16x2 blocks3 Cv12 composed1 packed0 fold1 lat1 8x24x40': [(2, 1, 849346560.0), (3, 1, 3397386240.0), (4, 1, 3397386240.0), (16, 2, 19660800.0), (22, 1, 2150400.0), (23, 1, 1474560.0)],
    'decode f32 blocks3 Cv24 composed0 packed0 fold1 lat1 8x24x40': [(14, 3, 10192158720.0), (15, 1, 21120.0), (17, 2, 15728640.0), (18, 1, 4116480.0), (26, 1, 3932160.0)],
    'decode bf16x3 blocks3 Cv24 composed0 packed0 fold0 lat1 8x24x40': [(10, 3, 10192158720.0), (15, 1, 21120.0), (16, 2, 19660800.0), (18, 1, 4116480.0), (25, 1, 5898240.0)],
    'decode bf16x3 blocks3 Cv24 composed0 packed0 fold1 lat1 8x24x40': [(10, 2, 6794772480.0), (11, 1, 3397386240.0), (15, 1, 21120.0), (16, 2, 19660800.0), (22, 1, 2150400.0), (25, 1, 5898240.0)],
    'decode f16x2 blocks3 Cv24 composed0 packed0 fold0 lat1 8x24x40': [(3, 3, 10192158720.0), (15, 1, 21120.0), (16, 2, 19660800.0), (18, 1, 4116480.0), (25, 1, 5898240.0)],
    'decode f16x2 blocks3 Cv24 composed0 packed0 fold1 lat1 8x24x40': [(3, 2, 6794772480.0), (4, 1, 3397386240.0), (15, 1, 21120.0), (16, 2, 19660800.0), (22, 1, 2150400.0), (25, 1, 5898240.0)],
    'decode f32 blocks1 Cv8 composed0 packed0 fold1 lat1 6x18x40': [(14, 1, 1911029760.0), (15, 1, 17280.0), (18, 1, 2315520.0), (26, 1, 2211840.0)],
    'decode bf16x3 blocks1 Cv8 composed0 packed0 fold0 lat1 6x18x40': [(10, 1, 1911029760.0), (15, 1, 17280.0), (18, 1, 2315520.0), (25, 1, 3317760.0)],
    'decode bf16x3 blocks1 Cv8 composed0 packed0 fold1 lat1 6x18x40': [(11, 1, 1911029760.0), (15, 1, 17280.0), (22, 1, 1209600.0), (25, 1, 3317760.0)],
    'decode bf16x3 blocks1 Cv8 composed1 packed0 fold0 lat1 6x18x40': [(8, 1, 477757440.0), (18, 1, 2315520.0), (24, 1, 829440.0)],
    'decode bf16x3 blocks1 Cv8 composed1 packed0 fold1 lat1 6x18x40': [(8, 1, 477757440.0), (18, 1, 2315520.0), (24, 1, 829440.0)],
    'decode bf16x3 blocks1 Cv8 composed1 packed1 fold0 lat1 6x18x40': [(6, 1, 247726080.0), (18, 1, 2315520.0), (24, 1, 829440.0)],
    'decode bf16x3 blocks1 Cv8 composed1 packed1 fold1 lat1 6x18x40': [(6, 1, 247726080.0), (18, 1, 2315520.0), (24, 1, 829440.0)],
    'decode f16x2 blocks1 Cv8 composed0 packed0 fold0 lat1 6x18x40': [(3, 1, 1911029760.0), (15, 1, 17280.0), (18, 1, 2315520.0), (25, 1, 3317760.0)],
    'decode f16x2 blocks1 Cv8 composed0 packed0 fold1 lat1 6x18x40': [(4, 1, 1911029760.0), (15, 1, 17280.0), (22, 1, 1209600.0), (25, 1, 3317760.0)],
    'decode f16x2 blocks1 Cv8 composed1 packed0 fold0 lat1 6x18x40': [(2, 1, 477757440.0), (18, 1, 2315520.0), (24, 1, 829440.0)],
    'decode f16x2 blocks1 Cv8 composed1 packed0 fold1 lat1 6x18x40': [(2, 1, 477757440.0), (18, 1, 2315520.0), (24, 1, 829440.0)],
    'decode f16x2 blocks1 Cv8 composed1 packed1 fold0 lat1 6x18x40': [(1, 1, 247726080.0), (18, 1, 2315520.0), (24, 1, 829440.0)],
    'decode f16x2 blocks1 Cv8 composed1 packed1 fold1 lat1 6x18x40': [(1, 1, 247726080.0), (18, 1, 2315520.0), (24, 1, 829440.0)],
    'decode f32 blocks1 Cv12 composed0 packed0 fold1 lat1 6x18x40': [(14, 1, 1911029760.0), (15, 1, 18240.0), (18, 1, 2315520.0), (26, 1, 2211840.0)],
    'decode bf16x3 blocks1 Cv12 composed0 packed0 fold0 lat1 6x18x40': [(10, 1, 1911029760.0), (15, 1, 18240.0), (18, 1, 2315520.0), (25, 1, 3317760.0)],
    'decode bf16x3 blocks1 Cv12 composed0 packed0 fold1 lat1 6x18x40': [(11, 1, 1911029760.0), (15, 1, 18240.0), (22, 1, 1209600.0), (25, 1, 3317760.0)],
    'decode bf16x3 blocks1 Cv12 composed1 packed0 fold0 lat1 6x18x40': [(8, 1, 477757440.0), (18, 1, 2315520.0), (23, 1, 829440.0)],
    'decode bf16x3 blocks1 Cv12 composed1 packed0 fold1 lat1 6x18x40': [(8, 1, 477757440.0), (18, 1, 2315520.0), (23, 1, 829440.0)],
    'decode f16x2 blocks1 Cv12 composed0 packed0 fold0 lat1 6x18x40': [(3, 1, 1911029760.0), (15, 1, 18240.0), (18, 1, 2315520.0), (25, 1, 3317760.0)],
    'decode f16x2 blocks1 Cv12 composed0 packed0 fold1 lat1 6x18x40': [(4, 1, 1911029760.0), (15, 1, 18240.0), (22, 1, 1209600.0), (25, 1, 3317760.0)],
    'decode f16x2 blocks1 Cv12 composed1 packed0 fold0 lat1 6x18x40': [(2, 1, 477757440.0), (18, 1, 2315520.0), (23, 1, 829440.0)],
    'decode f16x2 blocks1 Cv12 composed1 packed0 fold1 lat1 6x18x40': [(2, 1, 477757440.0), (18, 1, 2315520.0), (23, 1, 829440.0)],
    'decode f32 blocks1 Cv24 composed0 packed0 fold1 lat1 6x18x40': [(14, 1, 1911029760.0), (15, 1, 21120.0), (18, 1, 2315520.0), (26, 1, 2211840.0)],
    'decode bf16x3 blocks1 Cv24 composed0 packed0 fold0 lat1 6x18x40': [(10, 1, 1911029760.0), (15, 1, 21120.0), (18, 1, 2315520.0), (25, 1, 3317760.0)],
    'decode bf16x3 blocks1 Cv24 composed0 packed0 fold1 lat1 6x18x40': [(11, 1, 1911029760.0), (15, 1, 21120.0), (22, 1, 1209600.0), (25, 1, 3317760.0)],
    'decode f16x2 blocks1 Cv24 composed0 packed0 fold0 lat1 6x18x40': [(3, 1, 1911029760.0), (15, 1, 21120.0), (18, 1, 2315520.0), (25, 1, 3317760.0)],
    'decode f16x2 blocks1 Cv24 composed0 packed0 fold1 lat1 6x18x40': [(4, 1, 1911029760.0), (15, 1, 21120.0), (22, 1, 1209600.0), (25, 1, 3317760.0)],
    'decode f32 blocks2 Cv8 composed0 packed0 fold1 lat1 6x18x40': [(14, 2, 3822059520.0), (15, 1, 17280.0), (17, 1, 4423680.0), (18, 1, 2315520.0), (26, 1, 2211840.0)],
    'decode bf16x3 blocks2 Cv8 composed0 packed0 fold0 lat1 6x18x40': [(10, 2, 3822059520.0), (15, 1, 17280.0), (16, 1, 5529600.0), (18, 1, 2315520.0), (25, 1, 3317760.0)],
    'decode bf16x3 blocks2 Cv8 composed0 packed0 fold1 lat1 6x18x40': [(10, 1, 1911029760.0), (11, 1, 1911029760.0), (15, 1, 17280.0), (16, 1, 5529600.0), (22, 1, 1209600.0), (25, 1, 3317760.0)],
    'decode bf16x3 blocks2 Cv8 composed1 packed0 fold0 lat1 6x18x40': [(8, 1, 477757440.0), (10, 1, 1911029760.0), (16, 1, 5529600.0), (18, 1, 2315520.0), (24, 1, 829440.0)],
    'decode bf16x3 blocks2 Cv8 composed1 packed0 fold1 lat1 6x18x40': [(0, 1, 2211840.0), (9, 1, 477757440.0), (11, 1, 1911029760.0), (22, 1, 1209600.0), (24, 1, 829440.0)],
    'decode bf16x3 blocks2 Cv8 composed1 packed1 fold0 lat1 6x18x40': [(6, 1, 247726080.0), (10, 1, 1911029760.0), (16, 1, 5529600.0), (18, 1, 2315520.0), (24, 1, 829440.0)],
    'decode bf16x3 blocks2 Cv8 composed1 packed1 fold1 lat1 6x18x40': [(0, 1, 2211840.0), (7, 1, 247726080.0), (11, 1, 1911029760.0), (22, 1, 1209600.0), (24, 1, 829440.0)],
    'decode f16x2 blocks2 Cv8 composed0 packed0 fold0 lat1 6x18x40': [(3, 2, 3822059520.0), (15, 1, 17280.0), (16, 1, 5529600.0), (18, 1, 2315520.0), (25, 1, 3317760.0)],
    'decode f16x2 blocks2 Cv8 composed0 packed0 fold1 lat1 6x18x40': [(3, 1, 1911029760.0), (4, 1, 1911029760.0), (15, 1, 17280.0), (16, 1, 5529600.0), (22, 1, 1209600.0), (25, 1, 3317760.0)],
    'decode f16x2 blocks2 Cv8 composed1 packed0 fold0 lat1 6x18x40': [(2, 1, 477757440.0), (3, 1, 1911029760.0), (16, 1, 5529600.0), (18, 1, 2315520.0), (24, 1, 829440.0)],
    'decode f16x2 blocks2 Cv8 composed1 packed0 fold1 lat1 6x18x40': [(2, 1, 477757440.0), (4, 1, 1911029760.0), (16, 1, 5529600.0), (22, 1, 1209600.0), (24, 1, 829440.0)],
    'decode f16x2 blocks2 Cv8 composed1 packed1 fold0 lat1 6x18x40': [(1, 1, 247726080.0), (3, 1, 1911029760.0), (16, 1, 5529600.0), (18, 1, 2315520.0), (24, 1, 829440.0)],
    'decode f16x2 blocks2 Cv8 composed1 packed1 fold1 lat1 6x18x40': [(1, 1, 247726080.0), (4, 1, 1911029760.0), (16, 1, 5529600.0), (22, 1, 1209600.0), (24, 1, 829440.0)],
    'decode f32 blocks2 Cv12 composed0 packed0 fold1 lat1 6x18x40': [(14, 2, 3822059520.0), (15, 1, 18240.0), (17, 1, 4423680.0), (18, 1, 2315520.0), (26, 1, 2211840.0)],
    'decode bf16x3 blocks2 Cv12 composed0 packed0 fold0 lat1 6x18x40': [(10, 2, 3822059520.0), (15, 1, 18240.0), (16, 1, 5529600.0), (18, 1, 2315520.0), (25, 1, 3317760.0)],
    'decode bf16x3 blocks2 Cv12 composed0 packed0 fold1 lat1 6x18x40': [(10, 1, 1911029760.0), (11, 1, 1911029760.0), (15, 1, 18240.0), (16, 1, 5529600.0), (22, 1, 1209600.0), (25, 1, 3317760.0)],
    'decode bf16x3 blocks2 Cv12 composed1 packed0 fold0 lat1 6x18x40': [(8, 1, 477757440.0), (10, 1, 1911029760.0), (16, 1, 5529600.0), (18, 1, 2315520.0), (23, 1, 829440.0)],
    'decode bf16x3 blocks2 Cv12 composed1 packed0 fold1 lat1 6x18x40': [(0, 1, 2211840.0), (9, 1, 477757440.0), (11, 1, 1911029760.0), (22, 1, 1209600.0), (23, 1, 829440.0)],
    'decode f16x2 blocks2 Cv12 composed0 packed0 fold0 lat1 6x18x40': [(3, 2, 3822059520.0), (15, 1, 18240.0), (16, 1, 5529600.0), (18, 1, 2315520.0), (25, 1, 3317760.0)],
    'decode f16x2 blocks2 Cv12 composed0 packed0 fold1 lat1 6x18x40': [(3, 1, 1911029760.0), (4, 1, 1911029760.0), (15, 1, 18240.0), (16, 1, 5529600.0), (22, 1, 1209600.0), (25, 1, 3317760.0)],
    'decode f16x2 blocks2 Cv12 composed1 packed0 fold0 lat1 6x18x40': [(2, 1, 477757440.0), (3, 1, 1911029760.0), (16, 1, 5529600.0), (18, 1, 2315520.0), (23, 1, 829440.0)],
    'decode f16x2 blocks2 Cv12 composed1 packed0 fold1 lat1 6x18x40': [(2, 1, 477757440.0), (4, 1, 1911029760.0), (16, 1, 5529600.0), (22, 1, 1209600.0), (23, 1, 829440.0)],
    'decode f32 blocks2 Cv24 composed0 packed0 fold1 lat1 6x18x40': [(14, 2, 3822059520.0), (15, 1, 21120.0), (17, 1, 4423680.0), (18, 1, 2315520.0), (26, 1, 2211840.0)],
    'decode bf16x3 blocks2 Cv24 composed0 packed0 fold0 lat1 6x18x40': [(10, 2, 3822059520.0), (15, 1, 21120.0), (16, 1, 5529600.0), (18, 1, 2315520.0), (25, 1, 3317760.0)],
    'decode bf16x3 blocks2 Cv24 composed0 packed0 fold1 lat1 6x18x40': [(10, 1, 1911029760.0), (11, 1, 1911029760.0), (15, 1, 21120.0), (16, 1, 5529600.0), (22, 1, 1209600.0), (25, 1, 3317760.0)],
    'decode f16x2 blocks2 Cv24 composed0 packed0 fold0 lat1 6x18x40': [(3, 2, 3822059520.0), (15, 1, 21120.0), (16, 1, 5529600.0), (18, 1, 2315520.0), (25, 1, 3317760.0)],
    'decode f16x2 blocks2 Cv24 composed0 packed0 fold1 lat1 6x18x40': [(3, 1, 1911029760.0), (4, 1, 1911029760.0), (15, 1, 21120.0), (16, 1, 5529600.0), (22, 1, 1209600.0), (25, 1, 3317760.0)],
    'decode f32 blocks3 Cv8 composed0 packed0 fold1 lat1 6x18x40': [(14, 3, 5733089280.0), (15, 1, 17280.0), (17, 2, 8847360.0), (18, 1, 2315520.0), (26, 1, 2211840.0)],
    'decode bf16x3 blocks3 Cv8 composed0 packed0 fold0 lat1 6x18x40': [(10, 3, 5733089280.0), (15, 1, 17280.0), (16, 2, 11059200.0), (18, 1, 2315520.0), (25, 1, 3317760.0)],
    'decode bf16x3 blocks3 Cv8 composed0 packed0 fold1 lat1 6x18x40': [(10, 2, 3822059520.0), (11, 1, 1911029760.0), (15, 1, 17280.0), (16, 2, 11059200.0), (22, 1, 1209600.0), (25, 1, 3317760.0)],
    'decode bf16x3 blocks3 Cv8 composed1 packed0 fold0 lat1 6x18x40': [(8, 1, 477757440.0), (10, 2, 3822059520.0), (16, 2, 11059200.0), (18, 1, 2315520.0), (24, 1, 829440.0)],
    'decode bf16x3 blocks3 Cv8 composed1 packed0 fold1 lat1 6x18x40': [(8, 1, 477757440.0), (10, 1, 1911029760.0), (11, 1, 1911029760.0), (16, 2, 11059200.0), (22, 1, 1209600.0), (24, 1, 829440.0)],
    'decode bf16x3 blocks3 Cv8 composed1 packed1 fold0 lat1 6x18x40': [(6, 1, 247726080.0), (10, 2, 3822059520.0), (16, 2, 11059200.0), (18, 1, 2315520.0), (24, 1, 829440.0)],
    'decode bf16x3 blocks3 Cv8 composed1 packed1 fold1 lat1 6x18x40': [(6, 1, 247726080.0), (10, 1, 1911029760.0), (11, 1, 1911029760.0), (16, 2, 11059200.0), (22, 1, 1209600.0), (24, 1, 829440.0)],
    'decode f16x2 blocks3 Cv8 composed0 packed0 fold0 lat1 6x18x40': [(3, 3, 5733089280.0), (15, 1, 17280.0), (16, 2, 11059200.0), (18, 1, 2315520.0), (25, 1, 3317760.0)],
    'decode f16x2 blocks3 Cv8 composed0 packed0 fold1 lat1 6x18x40': [(3, 2, 3822059520.0), (4, 1, 1911029760.0), (15, 1, 17280.0), (16, 2, 11059200.0), (22, 1, 1209600.0), (25, 1, 3317760.0)],
    'decode f16x2 blocks3 Cv8 composed1 packed0 fold0 lat1 6x18x40': [(2, 1, 477757440.0), (3, 2, 3822059520.0), (16, 2, 11059200.0), (18, 1, 2315520.0), (24, 1, 829440.0)],
    'decode f16x2 blocks3 Cv8 composed1 packed0 fold1 lat1 6x18x40': [(2, 1, 477757440.0), (3, 1, 1911029760.0), (4, 1, 1911029760.0), (16, 2, 11059200.0), (22, 1, 1209600.0), (24, 1, 829440.0)],
    'decode f16x2 blocks3 Cv8 composed1 packed1 fold0 lat1 6x18x40': [(1, 1, 247726080.0), (3, 2, 3822059520.0), (16, 2, 11059200.0), (18, 1, 2315520.0), (24, 1, 829440.0)],
    'decode f16x2 blocks3 Cv8 composed1 packed1 fold1 lat1 6x18x40': [(1, 1, 247726080.0), (3, 1, 1911029760.0), (4, 1, 1911029760.0), (16, 2, 11059200.0), (22, 1, 1209600.0), (24, 1, 829440.0)],
    'decode f32 blocks3 Cv12 composed0 packed0 fold1 lat1 6x18x40': [(14, 3, 5733089280.0), (15, 1, 18240.0), (17, 2, 8847360.0), (18, 1, 2315520.0), (26, 1, 2211840.0)],
    'decode bf16x3 blocks3 Cv12 composed0 packed0 fold0 lat1 6x18x40': [(10, 3, 5733089280.0), (15, 1, 18240.0), (16, 2, 11059200.0), (18, 1, 2315520.0), (25, 1, 3317760.0)],
    'decode bf16x3 blocks3 Cv12 composed0 packed0 fold1 lat1 6x18x40': [(10, 2, 3822059520.0), (11, 1, 1911029760.0), (15, 1, 18240.0), (16, 2, 11059200.0), (22, 1, 1209600.0), (25, 1, 3317760.0)],
    'decode bf16x3 blocks3 Cv12 composed1 packed0 fold0 lat1 6x18x40': [(8, 1, 477757440.0), (10, 2, 3822059520.0), (16, 2, 11059200.0), (18, 1, 2315520.0), (23, 1, 829440.0)],
    'decode bf16x3 blocks3 Cv12 composed1 packed0 fold1 lat1 6x18x40': [(8, 1, 477757440.0), (10, 1, 1911029760.0), (11, 1, 1911029760.0), (16, 2, 11059200.0), (22, 1, 1209600.0), (23, 1, 829440.0)],
    'decode f16x2 blocks3 Cv12 composed0 packed0 fold0 lat1 6x18x40': [(3, 3, 5733089280.0), (15, 1, 18240.0), (16, 2, 11059200.0), (18, 1, 2315520.0), (25, 1, 3317760.0)],
    'decode f16x2 blocks3 Cv12 composed0 packed0 fold1 lat1 6x18x40': [(3, 2, 3822059520.0), (4, 1, 1911029760.0), (15, 1, 18240.0), (16, 2, 11059200.0), (22, 1, 1209600.0), (25, 1, 3317760.0)],
    'decode f16x2 blocks3 Cv12 composed1 packed0 fold0 lat1 6x18x40': [(2, 1, 477757440.0), (3, 2, 3822059520.0), (16, 2, 11059200.0), (18, 1, 2315520.0), (23, 1, 829440.0)],
    'decode f16x2 blocks3 Cv12 composed1 packed0 fold1 lat1 6x18x40': [(2, 1, 477757440.0), (3, 1, 1911029760.0), (4, 1, 1911029760.0), (16, 2, 11059200.0), (22, 1, 1209600.0), (23, 1, 829440.0)],
    'decode f32 blocks3 Cv24 composed0 packed0 fold1 lat1 6x18x40': [(14, 3, 5733089280.0), (15, 1, 21120.0), (17, 2, 8847360.0), (18, 1, 2315520.0), (26, 1, 2211840.0)],
    'decode bf16x3 blocks3 Cv24 composed0 packed0 fold0 lat1 6x18x40': [(10, 3, 5733089280.0), (15, 1, 21120.0), (16, 2, 11059200.0), (18, 1, 2315520.0), (25, 1, 3317760.0)],
    'decode bf16x3 blocks3 Cv24 composed0 packed0 fold1 lat1 6x18x40': [(10, 2, 3822059520.0), (11, 1, 1911029760.0), (15, 1, 21120.0), (16, 2, 11059200.0), (22, 1, 1209600.0), (25, 1, 3317760.0)],
    'decode f16x2 blocks3 Cv24 composed0 packed0 fold0 lat1 6x18x40': [(3, 3, 5733089280.0), (15, 1, 21120.0), (16, 2, 11059200.0), (18, 1, 2315520.0), (25, 1, 3317760.0)],
    'decode f16x2 blocks3 Cv24 composed0 packed0 fold1 lat1 6x18x40': [(3, 2, 3822059520.0), (4, 1, 1911029760.0), (15, 1, 21120.0), (16, 2, 11059200.0), (22, 1, 1209600.0), (25, 1, 3317760.0)],
    'decode f32 blocks2 Cv8 composed1 packed1 fold1 lat0 8x24x40': [(14, 2, 6794772480.0), (15, 1, 17280.0), (17, 1, 7864320.0), (18, 1, 4116480.0), (26, 1, 3932160.0)],
    'decode bf16x3 blocks2 Cv8 composed1 packed1 fold1 lat0 8x24x40': [(10, 1, 3397386240.0), (11, 1, 3397386240.0), (15, 1, 17280.0), (16, 1, 9830400.0), (22, 1, 2150400.0), (25, 1, 5898240.0)],
    'decode f16x2 blocks2 Cv8 composed1 packed1 fold1 lat0 8x24x40': [(3, 1, 3397386240.0), (4, 1, 3397386240.0), (15, 1, 17280.0), (16, 1, 9830400.0), (22, 1, 2150400.0), (25, 1, 5898240.0)],
    'encode f32 blocks1 packed0 fold1 pool488': [(13, 1, 63700992.0), (19, 1, 1572864.0)],
    'encode bf16x3 blocks1 packed0 fold1 pool488': [(13, 1, 63700992.0), (19, 1, 1572864.0)],
    'encode f16x2 blocks1 packed0 fold1 pool488': [(13, 1, 63700992.0), (19, 1, 1572864.0)],
    'encode f32 blocks2 packed0 fold1 pool488': [(13, 1, 63700992.0), (14, 1, 1358954496.0), (17, 1, 3145728.0), (19, 1, 1572864.0)],
    'encode bf16x3 blocks2 packed0 fold0 pool488': [(10, 1, 1358954496.0), (13, 1, 63700992.0), (16, 1, 3932160.0), (19, 1, 1572864.0)],
    'encode bf16x3 blocks2 packed0 fold1 pool488': [(12, 1, 1358954496.0), (13, 1, 63700992.0), (16, 1, 3932160.0), (20, 1, 49152.0)],
    'encode bf16x3 blocks2 packed1 fold0 pool488': [(10, 1, 1358954496.0), (13, 1, 63700992.0), (16, 1, 3932160.0), (19, 1, 1572864.0)],
    'encode bf16x3 blocks2 packed1 fold1 pool488': [(0, 1, 2211840.0), (7, 1, 176160768.0), (12, 1, 1358954496.0), (20, 1, 49152.0), (21, 1, 663552.0)],
    'encode f16x2 blocks2 packed0 fold0 pool488': [(3, 1, 1358954496.0), (13, 1, 63700992.0), (16, 1, 3932160.0), (19, 1, 1572864.0)],
    'encode f16x2 blocks2 packed0 fold1 pool488': [(5, 1, 1358954496.0), (13, 1, 63700992.0), (16, 1, 3932160.0), (20, 1, 49152.0)],
    'encode f32 blocks3 packed0 fold1 pool488': [(13, 1, 63700992.0), (14, 2, 2717908992.0), (17, 2, 6291456.0), (19, 1, 1572864.0)],
    'encode bf16x3 blocks3 packed0 fold0 pool488': [(10, 2, 2717908992.0), (13, 1, 63700992.0), (16, 2, 7864320.0), (19, 1, 1572864.0)],
    'encode bf16x3 blocks3 packed0 fold1 pool488': [(10, 1, 1358954496.0), (12, 1, 1358954496.0), (13, 1, 63700992.0), (16, 2, 7864320.0), (20, 1, 49152.0)],
    'encode f16x2 blocks3 packed0 fold0 pool488': [(3, 2, 2717908992.0), (13, 1, 63700992.0), (16, 2, 7864320.0), (19, 1, 1572864.0)],
    'encode f16x2 blocks3 packed0 fold1 pool488': [(3, 1, 1358954496.0), (5, 1, 1358954496.0), (13, 1, 63700992.0), (16, 2, 7864320.0), (20, 1, 49152.0)],
    'encode f32 blocks1 packed0 fold1 pool244': [(13, 1, 29859840.0), (19, 1, 737280.0)],
    'encode bf16x3 blocks1 packed0 fold1 pool244': [(13, 1, 29859840.0), (19, 1, 737280.0)],
    'encode f16x2 blocks1 packed0 fold1 pool244': [(13, 1, 29859840.0), (19, 1, 737280.0)],
    'encode f32 blocks2 packed0 fold1 pool244': [(13, 1, 29859840.0), (14, 1, 637009920.0), (17, 1, 1474560.0), (19, 1, 737280.0)],
    'encode bf16x3 blocks2 packed0 fold0 pool244': [(10, 1, 637009920.0), (13, 1, 29859840.0), (16, 1, 1843200.0), (19, 1, 737280.0)],
    'encode bf16x3 blocks2 packed0 fold1 pool244': [(10, 1, 637009920.0), (13, 1, 29859840.0), (16, 1, 1843200.0), (19, 1, 737280.0)],
    'encode bf16x3 blocks2 packed1 fold0 pool244': [(10, 1, 637009920.0), (13, 1, 29859840.0), (16, 1, 1843200.0), (19, 1, 737280.0)],
    'encode bf16x3 blocks2 packed1 fold1 pool244': [(10, 1, 637009920.0), (13, 1, 29859840.0), (16, 1, 1843200.0), (19, 1, 737280.0)],
    'encode f16x2 blocks2 packed0 fold0 pool244': [(3, 1, 637009920.0), (13, 1, 29859840.0), (16, 1, 1843200.0), (19, 1, 737280.0)],
    'encode f16x2 blocks2 packed0 fold1 pool244': [(3, 1, 637009920.0), (13, 1, 29859840.0), (16, 1, 1843200.0), (19, 1, 737280.0)],
    'encode f32 blocks3 packed0 fold1 pool244': [(13, 1, 29859840.0), (14, 2, 1274019840.0), (17, 2, 2949120.0), (19, 1, 737280.0)],
    'encode bf16x3 blocks3 packed0 fold0 pool244': [(10, 2, 1274019840.0), (13, 1, 29859840.0), (16, 2, 3686400.0), (19, 1, 737280.0)],
    'encode bf16x3 blocks3 packed0 fold1 pool244': [(10, 2, 1274019840.0), (13, 1, 29859840.0), (16, 2, 3686400.0), (19, 1, 737280.0)],
    'encode f16x2 blocks3 packed0 fold0 pool244': [(3, 2, 1274019840.0), (13, 1, 29859840.0), (16, 2, 3686400.0), (19, 1, 737280.0)],
    'encode f16x2 blocks3 packed0 fold1 pool244': [(3, 2, 1274019840.0), (13, 1, 29859840.0), (16, 2, 3686400.0), (19, 1, 737280.0)],
}
