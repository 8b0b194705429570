"""Guidance interval, host side: the schedule segmentation, argument checks, config-key parsing, and the numpy mirror of the cond-only
update against the project's DDIM / DPM references fed eps_cond."""
import numpy as np
import pytest
import torch

import _dpm_ref as D
import _interval_ref as IR
import _noise_ref as N
from oracle import ref_cpu as R

ABAR = R.alpha_bar_table(R.beta_table(1000))


def _segs(sched, interval):
    from multimodal_diffusion_amd import schedule_utils as su
    return su.guidance_segments(sched, interval)


def _check_partition(segs, n):
    assert segs[0][0] == 0 and segs[-1][1] == n
    assert all(a[1] == b[0] for a, b in zip(segs, segs[1:]))                 # contiguous, in order
    assert all(a < b for a, b, _ in segs)
    assert all(a[2] != b[2] for a, b in zip(segs, segs[1:]))                 # maximal runs
    assert [i for a, b, _ in segs for i in range(a, b)] == list(range(n))


def test_segments_cases():
    sched = R.sampling_schedule(1000, 10)                                     # 999, 899, ..., 99, -1
    assert sched.tolist() == [999, 899, 799, 699, 599, 499, 399, 299, 199, 99, -1]
    assert _segs(sched, None) == [(0, 10, True)]
    assert _segs(sched, (0, 999)) == [(0, 10, True)]                          # covers the schedule: one CFG segment
    assert _segs(sched, (0, 5000)) == [(0, 10, True)]
    assert _segs(sched, (1000, 2000)) == [(0, 10, False)]                     # disjoint: one cond-only segment
    assert _segs(sched, (300, 398)) == [(0, 10, False)]                       # between two entries: contains no timestep
    assert _segs(sched, (300, 700)) == [(0, 3, False), (3, 7, True), (7, 10, False)]
    # both ends inclusive
    assert _segs(sched, (299, 699)) == [(0, 3, False), (3, 8, True), (8, 10, False)]
    assert _segs(sched, (300, 698)) == [(0, 4, False), (4, 7, True), (7, 10, False)]
    # single-step segments
    assert _segs(sched, (599, 599)) == [(0, 4, False), (4, 5, True), (5, 10, False)]
    assert _segs(sched, (999, 999)) == [(0, 1, True), (1, 10, False)]
    assert _segs(sched, (0, 99)) == [(0, 9, False), (9, 10, True)]
    # the final entry (-1) starts no step: it never makes a segment
    assert _segs(torch.tensor([5, -1]), (0, 10)) == [(0, 1, True)]
    assert _segs(torch.tensor([5]), (0, 10)) == []
    # a non-monotonic schedule alternates
    assert _segs([900, 100, 800, 50, -1], (500, 1000)) == [(0, 1, True), (1, 2, False), (2, 3, True), (3, 4, False)]


@pytest.mark.parametrize("n", [1, 2, 7, 50])
def test_segments_partition_and_kinds(n):
    sched = R.sampling_schedule(1000, n)
    rng = np.random.default_rng(n)
    for _ in range(40):
        lo = int(rng.integers(0, 1100))
        hi = int(rng.integers(lo, 1200))
        segs = _segs(sched, (lo, hi))
        _check_partition(segs, n)
        kinds = IR.step_kinds(sched, (lo, hi))
        assert [c for a, b, c in segs for _ in range(a, b)] == kinds


def test_interval_argument_checks():
    from multimodal_diffusion_amd import schedule_utils as su
    assert su.check_guidance_interval(None) is None
    assert su.check_guidance_interval((200, 800)) == (200, 800)
    assert su.check_guidance_interval([0, 0]) == (0, 0)
    assert su.check_guidance_interval((np.int64(3), torch.tensor(9))) == (3, 9)
    for bad in ((800, 200), (-1, 5), (-5, -2), (1.5, 9), (1, 9.0), ("1", "9"), (1,), (1, 2, 3), 5, "ab", (True, 3)):
        with pytest.raises(ValueError, match="guidance_interval"):
            su.check_guidance_interval(bad)
        with pytest.raises(ValueError, match="guidance_interval"):
            su.guidance_segments(R.sampling_schedule(1000, 4), bad)


def test_config_key_parsing():
    from multimodal_diffusion_amd import schedule_utils as su
    scfg = {"guidance_scale": {"video": 3.0}, "guidance_interval": {"video": [200, 800], "audio": (0, 500)}}
    assert su.guidance_interval_from_config(scfg, "video") == (200, 800)
    assert su.guidance_interval_from_config(scfg, "audio") == (0, 500)
    assert su.guidance_interval_from_config({"guidance_interval": {"video": [1, 2]}}, "audio") is None
    assert su.guidance_interval_from_config({}, "video") is None
    assert su.guidance_interval_from_config({"guidance_interval": None}, "video") is None
    for bad in ({"guidance_interval": [200, 800]}, {"guidance_interval": {"video": [800, 200]}}, {"guidance_interval": {"video": [1.5, 3]}}):
        with pytest.raises(ValueError, match="guidance_interval"):
            su.guidance_interval_from_config(bad, "video")


def test_engine_and_entry_points_take_the_interval():
    """the keyword exists at every level (the engine itself needs a device: its checks run through check_guidance_interval)"""
    import inspect
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import stream_infer as S
    assert inspect.signature(A.DenoiseEngine.__init__).parameters["guidance_interval"].default is None
    assert inspect.signature(A.DenoiseEngine.step).parameters["cond_only"].default is False
    assert inspect.signature(A.DenoiseEngine.advance).parameters["cond_only"].default is False
    assert "interval" in inspect.signature(A.DenoiseEngine.set_guidance_interval).parameters
    assert inspect.signature(A.sample_one_direction).parameters["guidance_interval"].default is None
    assert inspect.signature(S.stream_generate).parameters["guidance_interval"].default is None


def _case(seed=0, B=3, per=257):
    g = torch.Generator().manual_seed(seed)
    x, ec, en = (torch.randn(B, per, generator=g) for _ in range(3))
    return x, ec, en


def test_cond_update_mirror_equals_ddim_reference():
    x, ec, en = _case()
    tn, tp = torch.tensor([981, 402, 40]), torch.tensor([961, 382, -1])
    for eta in (0.0, 0.7):
        noise = None if eta == 0 else torch.from_numpy(N.normals(11, 5, tn.numpy(), x.shape[1])).float()
        ref = R.ddim_update(x.double(), tn, tp, ec.double(), ABAR.double(), eta, None if noise is None else noise.double()).numpy()
        got, _ = IR.cond_update_f64(x.numpy(), ec.numpy(), ABAR.numpy(), tn.tolist(), tp.tolist(), eta=eta,
                                    noise=None if noise is None else noise.numpy())
        assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
        # it is the oracle's CFG step at guidance 1 up to the combine's rounding (e_n + 1 (e_c - e_n) = e_c in real arithmetic)
        at1 = R.ddim_update(x.double(), tn, tp, (en + 1.0 * (ec - en)).double(), ABAR.double(), eta,
                            None if noise is None else noise.double()).numpy()
        assert np.abs(got - at1).max() <= 1e-5 * max(1.0, np.abs(ref).max())
        # and it ignores the null branch altogether: any other guidance moves the result
        at3 = R.ddim_update(x.double(), tn, tp, (en + 3.0 * (ec - en)).double(), ABAR.double(), eta,
                            None if noise is None else noise.double()).numpy()
        assert np.abs(got - at3).max() > 1e-2


def test_cond_update_mirror_equals_dpm_reference():
    x, ec, _ = _case(seed=1)
    h = torch.randn(x.shape, generator=torch.Generator().manual_seed(2))
    tl, tn, tp = [-1, 981, 700], [981, 402, 40], [961, 382, -1]          # first order, second order, final step
    ref, x0 = D.step_f64(x.numpy(), ec.numpy(), h.numpy(), ABAR.numpy(), tl, tn, tp)
    got, gx0 = IR.cond_update_f64(x.numpy(), ec.numpy(), ABAR.numpy(), tn, tp, solver="dpmpp_2m", x0_hist=h.numpy(), t_last=tl)
    assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    assert np.abs(gx0 - x0).max() <= 1e-12 * max(1.0, np.abs(x0).max())
    # the fp32 mirror of the kernels agrees to fp32 level
    f32, _ = D.step_f32(x.numpy(), ec.numpy(), h.numpy(), ABAR.numpy(), tl, tn, tp)
    assert np.abs(f32 - got).max() <= 1e-5 * max(1.0, np.abs(got).max())


def test_header_and_binding_list_the_new_entries():
    from multimodal_diffusion_amd import _lib as L
    hdr = (__import__("pathlib").Path(L.__file__).resolve().parent.parent / "include" / "avdiff_hip.h").read_text()
    for name in ("avd_denoise_step_cond_f32", "avd_eps_unpatch_ddim_f32", "avd_eps_untoken_ddim_audio_f32", "avd_embed_cond_f32"):
        assert name in L.SIGNATURES and f"int {name}(" in hdr
    assert L.ABI_VERSION == 7 and "#define AVD_ABI_VERSION 7" in hdr
