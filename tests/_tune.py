"""The library's process-wide tune keys (avd_tune_set) for the tests: their defaults, a setter, and a context manager that puts
every key it touched back to its default."""
from contextlib import contextmanager

import pytest

# the value each key has in a fresh process with no AVD_* environment override (the definitions of the g_* variables in csrc/)
DEFAULTS = {"gemm_tile": -1, "gemm_stages": 0, "s3_tile": -1, "s3_stagger": -1, "s3_min_rows": -1, "no_fold": 0, "s3_m16": 1,
            "s3_rt": 0, "s3_rt4": 0, "s3_deep4": 1, "s3_w128": 1, "s3_splitk": 4, "attn_pipe": 1, "core_trim": 1, "mlp_fused": 0, "gemm_splitk": 4,
            "attn_m16": 1, "cfg_rows": 1, "vae_lat": 1, "vae_fold": 1, "codec_mfma": 1, "s3_sn": 0, "s3_super4": 0, "s3_super8": 0}


def tune(key, value):
    from multimodal_diffusion_amd import _lib as L
    assert key in DEFAULTS, key
    L.check(L.lib().avd_tune_set(key.encode(), value))


@contextmanager
def tuned(*names, **keys):
    """sets the keys given with a value; on exit every key given, with a value or by name only, is back at its default (by name:
    a key that the block sets itself with tune(), in a loop for instance)"""
    try:
        for k, v in keys.items():
            tune(k, v)
        yield
    finally:
        for k in (*names, *keys):
            tune(k, DEFAULTS[k])


@pytest.fixture
def cfg_rows():
    """a setter of the "cfg_rows" key for one test; the default (1) is back afterwards.  Imported by the test modules that use it."""
    with tuned("cfg_rows"):
        yield lambda v: tune("cfg_rows", v)
