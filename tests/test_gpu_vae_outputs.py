"""What the VideoVAE routes compute (csrc/vae3d_f32.hip): every case of tests/test_gpu_vae_routes.py, which pins the kernels a case
runs, and the configurations the plans accept beyond them, against the fp64 oracle (oracle/ref_cpu.py: vae_decode, vae_encode) computed
live on the CPU.

Weights: one seeded set per configuration, loaded with load_state_dict, with every term a fold or a table carries non-trivial: conv
weights uniform +-1/sqrt(fan_in), conv biases N(0, 0.5^2), GroupNorm weight and bias N(0, 1), from_lat.bias = linspace(-1, 1, 64).
Inputs: batch 2, sample 1 scaled by 4, so that the two samples have different GroupNorm statistics and, on the f16x2 route, first images
whose device-derived scales are two binades apart.

Bounds, both asserted, on conftest.rel_err (max |difference| / max(1, max |reference|)):
  err < TOL                 the project's 1e-4
  err <= m e32 + floor      e32 = rel_err of the SAME oracle function evaluated in fp32 on the CPU (same weights and input) against its
                            fp64 result: what fp32 arithmetic delivers for these weights.  m = 8, floor = 1e-6 for "f32" and "bf16x3" (both
                            sides accumulate the same 64 x 27 fp32 products per output in different orders; the project's cross-route
                            checks allow 2 - 3 x between routes; 8 x leaves room for three stacked blocks); m = 16, floor = 2e-6 for
                            "f16x2", whose operands carry 22 mantissa bits instead of 24.
The call with max_workspace_bytes = 1 (one sample per launch) must return the bits of the batched call: per-sample statistics, weight
images, bias tables and image scales must not depend on what else is in the batch.  (With one first-image scale per LAUNCH the f16x2
decoder missed this by one ulp in "decode f16x2 blocks3 Cv8 composed1 packed1 fold0 / fold1 lat1 6x18x40": elements of sample 0 more than
17 binades below sample 1's maximum lost low-plane bits that they keep at their own scale.)"""
import re

import pytest
import torch

from _kit import dev  # noqa: F401  (fixture)
from _tune import tuned
from conftest import rel_err
from oracle import ref_cpu as R
from test_gpu_parity import TOL
from test_gpu_vae_routes import DEC_OUT, ENC_IN, MODES, _case_id, _cases

pytestmark = pytest.mark.gpu

MARGIN = {"f32": (8.0, 1e-6), "bf16x3": (8.0, 1e-6), "f16x2": (16.0, 2e-6)}        # mode -> (m, floor)
# (mode, vae_fold) of the small cases: "f32" does not read the switch
SWEEP = [("f32", 1), ("bf16x3", 0), ("bf16x3", 1), ("f16x2", 0), ("f16x2", 1)]


def _weights(vae, seed):
    """a state_dict for `vae` drawn from one generator, in the order of its keys"""
    g = torch.Generator().manual_seed(seed)
    W = {}
    for k, p in vae.state_dict().items():
        if re.search(r"_net\.\d+\.2\.", k):                              # GroupNorm weight and bias
            W[k] = torch.randn(p.shape, generator=g)
        elif p.dim() == 5:                                              # 3x3x3 and 1x1x1 convolutions
            W[k] = (torch.rand(p.shape, generator=g) * 2 - 1) / (p[0].numel() ** 0.5)
        else:
            W[k] = 0.5 * torch.randn(p.shape, generator=g)
    W["from_lat.bias"] = torch.linspace(-1, 1, W["from_lat.bias"].numel())
    return W


class _Runner:
    """modules with the seeded weights, their inputs, and the oracle's result per (weights, input, output size), each computed once"""

    def __init__(self, dev):
        from multimodal_diffusion_amd import _lib as L
        self.dev, self.L = dev, L
        self.vaes, self.inputs, self.refs = {}, {}, {}
        self.worst = {}                  # mode -> [(err, case), (err / e32, case)]

    def fresh(self, nb, cv, t_down, s_down, in_ch=3, act="sigmoid", variational=False):
        """-> (a new module on the device, its weights on the CPU)"""
        import multimodal_diffusion_amd as A
        cfg = A.VideoVAEConfig(in_ch=in_ch, lat_ch=cv, t_down=t_down, s_down=s_down, enc_blocks=nb, dec_blocks=nb, variational=variational,
                               out_activation=act)
        vae = A.VideoVAE(cfg).eval()
        W = _weights(vae, 100000 * in_ch + 1000 * nb + 10 * cv + t_down)
        vae.load_state_dict(W, strict=True)
        return vae.to(self.dev), W

    def vae(self, *key, **kw):
        full = key + tuple(sorted(kw.items()))
        if full not in self.vaes:
            self.vaes[full] = self.fresh(*key, **kw) + (full,)
        return self.vaes[full]

    def input(self, *shape):
        """[B, ...] from one generator per shape, sample 1 (if any) four times as large -> (on the device, on the CPU)"""
        if shape not in self.inputs:
            x = torch.randn(*shape, generator=torch.Generator().manual_seed(sum(shape)))
            if shape[0] > 1:
                x[1] *= 4
            self.inputs[shape] = (x.to(self.dev), x)
        return self.inputs[shape]

    def reference(self, key, fn):
        """fn(dtype) -> the oracle's output (a tuple: its first entry is compared); -> (fp64 result, e32)"""
        if key not in self.refs:
            r64, r32 = fn(torch.float64), fn(torch.float32)
            first = (lambda r: r[0] if isinstance(r, tuple) else r)
            self.refs[key] = (r64, rel_err(first(r32), first(r64)))
        return self.refs[key]

    def decode_ref(self, W, wkey, x, cfg, out_size):
        def fn(dt):
            return R.vae_decode(x.to(dt), {k: v.to(dt) for k, v in W.items()}, cfg.t_down, cfg.s_down, cfg.dec_blocks, cfg.out_activation, out_size)
        return self.reference(("dec", wkey, tuple(x.shape), out_size), fn)

    def encode_ref(self, W, wkey, x, cfg):
        def fn(dt):
            return R.vae_encode(x.to(dt), {k: v.to(dt) for k, v in W.items()}, cfg.t_down, cfg.s_down, cfg.enc_blocks, cfg.variational)
        return self.reference(("enc", wkey, tuple(x.shape)), fn)

    def judge(self, name, mode, out, ref, e32):
        """-> None, or what is wrong with `out`; keeps the worst figures per mode"""
        err = rel_err(out.cpu(), ref)
        m, floor = MARGIN[mode]
        w = self.worst.setdefault(mode, [(0.0, ""), (0.0, "")])
        w[0], w[1] = max(w[0], (err, name)), max(w[1], (err / max(e32, 1e-30), name))
        if not (err < TOL and err <= m * e32 + floor):
            return f"err {err:.3e} > min({TOL:g}, {m:g} x e32 {e32:.3e} + {floor:g})"
        return None

    def report(self, what):
        for mode, ((err, c0), (ratio, c1)) in sorted(self.worst.items()):
            print(f"[vae outputs] {what} {mode}: worst err {err:.3e} ({c0}); worst err / e32 {ratio:.2f} ({c1})")
        self.worst = {}

    def tags(self, call):
        """the profiling tags of one call (after one unrecorded call that caches the weight images)"""
        call()
        self.L.prof_enable(True)
        try:
            call()
            torch.cuda.synchronize()
        finally:
            self.L.prof_enable(False)
        return {k for k, v in self.L.prof_report().items() if v[0] > 0}

    # ---- one case of the routes file
    def matrix_case(self, case):
        if case[0] == "decode":
            _, mode, nb, cv, lc, lp, fold, lat, shape = case
            vae, W, wkey = self.vae(nb, cv, 4, 8)
            vae.matmul, vae.lat_composed, vae.lat_packed = mode, lc, lp
            x, x_cpu = self.input(2, cv, 2, 3, 5)
            ref, e32 = self.decode_ref(W, wkey, x_cpu, vae.cfg, DEC_OUT[shape])
            call, keys = (lambda **kw: vae.decode(x, out_size=DEC_OUT[shape], **kw)), dict(vae_fold=fold, vae_lat=lat)
        else:
            _, mode, nb, pk, fold, shape = case
            (T, H, Wd), (td, sd) = ENC_IN[shape]
            vae, W, wkey = self.vae(nb, 8, td, sd)
            vae.matmul, vae.enc_packed = mode, pk
            x, x_cpu = self.input(2, 3, T, H, Wd)
            ref, e32 = self.encode_ref(W, wkey, x_cpu, vae.cfg)
            call, keys = (lambda **kw: vae.encode(x, **kw)), dict(vae_fold=fold)
        with tuned(**keys):
            out, one = call(), call(max_workspace_bytes=1)
        bad = self.judge(_case_id(case), mode, out, ref, e32)
        if bad is None and not torch.equal(out, one):
            bad = f"one sample per launch differs from the batched call by {float((out - one).abs().max()):.3e}"
        return bad

    # ---- the small cases: one module, every (mode, vae_fold)
    def sweep(self, name, vae, call, ref, e32, check=None):
        """-> {case: what is wrong}; check(mode, fold, call) -> None or a complaint, run after the comparison"""
        wrong = {}
        for mode, fold in SWEEP:
            vae.matmul = mode
            with tuned(vae_fold=fold):
                out = call()
                bad = self.judge(f"{name} {mode} fold{fold}", mode, out, ref, e32)
                if bad is None and check is not None:
                    bad = check(mode, fold, out)
            if bad is not None:
                wrong[f"{name} {mode} fold{fold}"] = bad
        return wrong


@pytest.fixture(scope="module")
def runner(dev):
    return _Runner(dev)


# ------------------------------------------------------------------------------------------------- A: the route matrix
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("direction", ["decode", "encode"])
def test_route_output_matches_the_oracle(runner, direction, mode):
    cases = [c for c in _cases() if c[0] == direction and c[1] == mode]
    assert cases
    wrong = {}
    for c in cases:
        bad = runner.matrix_case(c)
        if bad is not None:
            wrong[_case_id(c)] = bad
    runner.report(f"{direction} matrix ({len(cases)} cases)")
    assert not wrong, wrong


ORDER = [("f32", True, True, 1), ("bf16x3", True, True, 1), ("bf16x3", True, True, 0), ("bf16x3", False, False, 0),
         ("f16x2", True, True, 1), ("f16x2", False, False, 1)]


@pytest.mark.parametrize("mode,lc,lp,fold", ORDER, ids=[f"{m}-composed{int(a)}-packed{int(b)}-fold{f}" for m, a, b, f in ORDER])
def test_smaller_shape_after_larger_reuses_the_workspace(runner, mode, lc, lp, fold):
    """8x24x40 then 6x18x40 through ONE module: the second call finds the first one's activations where its own halo belongs, and must
    return the bits of a fresh module (the halo zeroing); likewise the encoder, 8x16x24 then 4x8x16"""
    x, _ = runner.input(2, 8, 2, 3, 5)
    v, _ = runner.input(2, 3, 8, 16, 24)
    v_small = v[:, :, :4, :8, :16].contiguous()
    used, _ = runner.fresh(2, 8, 4, 8)
    new, _ = runner.fresh(2, 8, 4, 8)
    for m in (used, new):
        m.matmul, m.lat_composed, m.lat_packed = mode, lc, lp
    with tuned(vae_fold=fold):
        used.decode(x, out_size=DEC_OUT["8x24x40"])
        assert torch.equal(used.decode(x, out_size=DEC_OUT["6x18x40"]), new.decode(x, out_size=DEC_OUT["6x18x40"]))
        new2, _ = runner.fresh(2, 8, 4, 8)
        new2.matmul = mode
        used.encode(v)
        assert torch.equal(used.encode(v_small), new2.encode(v_small))


# ------------------------------------------------------------------------------------------------- B: accepted, never launched
def _composed(tags):
    """the latent-composed instantiations of the halo-tile conv among the tags: NSLAB (the second template argument) 1, or 0 = packed taps"""
    hits = [re.fullmatch(r"conv3d_k3_bf16x3_kernel<(\d+), (\d+), (\d+)>", t) for t in tags]
    return {int(h.group(2)) for h in hits if h and int(h.group(2)) <= 1}


@pytest.mark.parametrize("cv", [3, 16, 17])
def test_decode_latent_widths(runner, cv):
    """16 = the last composed width (a full 16-channel slab), 17 = the first that is not composed, 3 pads the packed 8-wide tap pairs"""
    vae, W, wkey = runner.vae(2, cv, 4, 8)
    x, x_cpu = runner.input(2, cv, 2, 3, 5)
    size = DEC_OUT["6x18x40"]
    ref, e32 = runner.decode_ref(W, wkey, x_cpu, vae.cfg, size)

    def route(mode, fold, out):
        if mode == "f32":
            return None
        tags = runner.tags(lambda: vae.decode(x, out_size=size))
        want = {3: {0}, 16: {1}, 17: set()}[cv]
        ups = {3: "upsample_lat8_kernel", 16: "upsample_lat16_kernel", 17: "fromlat_kernel"}[cv]
        others = {"upsample_lat8_kernel", "upsample_lat16_kernel", "fromlat_kernel"} - {ups}
        if _composed(tags) != want or ups not in tags or tags & others:
            return f"ran {sorted(tags)}"
        return None

    wrong = runner.sweep(f"decode Cv{cv}", vae, lambda: vae.decode(x, out_size=size), ref, e32, route)
    runner.report(f"decode Cv{cv}")
    assert not wrong, wrong


@pytest.mark.parametrize("act", ["sigmoid", "tanh"])
@pytest.mark.parametrize("ch", [1, 2, 4])
def test_decode_image_channels(runner, ch, act):
    """out_ch 1, 2, 4: gn_apply_toimg_kernel, and toimg_from_p_kernel with its wg / consts tables when vae_fold is on"""
    vae, W, wkey = runner.vae(2, 8, 4, 8, in_ch=ch, act=act)
    x, x_cpu = runner.input(2, 8, 2, 3, 5)
    size = DEC_OUT["6x18x40"]
    ref, e32 = runner.decode_ref(W, wkey, x_cpu, vae.cfg, size)
    assert ref.shape == (2, ch, 6, 18, 40)

    def shape(mode, fold, out):
        return None if out.shape == ref.shape else f"shape {tuple(out.shape)}"

    wrong = runner.sweep(f"decode out_ch{ch} {act}", vae, lambda: vae.decode(x, out_size=size), ref, e32, shape)
    runner.report(f"decode out_ch{ch} {act}")
    assert not wrong, wrong


@pytest.mark.parametrize("pool", list(ENC_IN))
@pytest.mark.parametrize("ch", [1, 2, 4])
def test_encode_image_channels(runner, ch, pool):
    """in_ch 1, 2, 4: rgb_to_ndhwc4_pad_kernel, and rgb_lat16_kernel with the packed first-conv image on the folded route"""
    (T, H, Wd), (td, sd) = ENC_IN[pool]
    vae, W, wkey = runner.vae(2, 8, td, sd, in_ch=ch)
    x, x_cpu = runner.input(2, ch, T, H, Wd)
    ref, e32 = runner.encode_ref(W, wkey, x_cpu, vae.cfg)
    wrong = runner.sweep(f"encode in_ch{ch} {pool}", vae, lambda: vae.encode(x), ref, e32)
    runner.report(f"encode in_ch{ch} {pool}")
    assert not wrong, wrong


@pytest.mark.parametrize("cv", [1, 5, 16])
def test_encode_latent_widths(runner, cv):
    (T, H, Wd), (td, sd) = ENC_IN["pool488"]
    vae, W, wkey = runner.vae(2, cv, td, sd)
    x, x_cpu = runner.input(2, 3, T, H, Wd)
    ref, e32 = runner.encode_ref(W, wkey, x_cpu, vae.cfg)
    assert ref.shape == (2, cv, 2, 2, 3)
    wrong = runner.sweep(f"encode lat_ch{cv}", vae, lambda: vae.encode(x), ref, e32)
    runner.report(f"encode lat_ch{cv}")
    assert not wrong, wrong


@pytest.mark.parametrize("pool", list(ENC_IN))
@pytest.mark.parametrize("nb", [1, 2, 3])
def test_variational_head(runner, nb, pool):
    """variational (eval), lat_ch 8: to_mu | to_logv as one 16-wide head on every route; z = mu and the KL term against the oracle's
    (1e-4 absolute, as test_dropin_corners_golden)"""
    (T, H, Wd), (td, sd) = ENC_IN[pool]
    vae, W, wkey = runner.vae(nb, 8, td, sd, variational=True)
    x, x_cpu = runner.input(2, 3, T, H, Wd)
    (mu, kld), e32 = runner.encode_ref(W, wkey, x_cpu, vae.cfg)

    def kl(mode, fold, out):
        got = float(vae.kld_loss())
        return None if abs(got - float(kld)) < 1e-4 else f"kld {got!r}, oracle {float(kld)!r}"

    wrong = runner.sweep(f"variational blocks{nb} {pool}", vae, lambda: vae.encode(x), mu, e32, kl)
    runner.report(f"variational blocks{nb} {pool}")
    assert not wrong, wrong


SIZES = {"3x3x5": ((1, 8, 1, 1, 1), (3, 3, 5)),          # smaller than one tile in every dimension: every voxel is a border voxel,
                                                         # every upsample source clamps
         "5x17x33": ((2, 8, 2, 3, 5), (5, 17, 33))}      # one voxel past a tile edge in each of T, H and W


@pytest.mark.parametrize("name", list(SIZES))
def test_decode_output_sizes(runner, name):
    zshape, size = SIZES[name]
    vae, W, wkey = runner.vae(2, 8, 4, 8)
    vae.lat_composed = vae.lat_packed = True
    x, x_cpu = runner.input(*zshape)
    ref, e32 = runner.decode_ref(W, wkey, x_cpu, vae.cfg, size)
    assert ref.shape[2:] == size
    wrong = runner.sweep(f"decode {name}", vae, lambda: vae.decode(x, out_size=size), ref, e32)
    vae.lat_composed = False
    wrong.update(runner.sweep(f"decode {name} composed0", vae, lambda: vae.decode(x, out_size=size), ref, e32))
    vae.lat_composed = True
    runner.report(f"decode {name}")
    assert not wrong, wrong
