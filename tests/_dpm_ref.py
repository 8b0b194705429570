"""numpy reference of the DPM-Solver++(2M) update (contract in include/avdiff_hip.h, avd_dpmpp_2m_step_f32).

Two forms:
  * ``coefs`` / ``x0_f32`` / ``step_f32``: the fp32 mirror of the kernels — coefficients in fp64 from the fp32 table, rounded once to
    fp32; x0 with DDIM's fp32 expression; the update in fp32 in the contract's order (numpy rounds every operation, no contraction);
  * ``step_f64``: the same solver in plain fp64 (trajectory tests and the convergence check of test_dpm_cpu.py).
"""
import math

import numpy as np


def _abar(abar, tau):
    """a(tau): alpha_bar[clamp(tau, 0, T-1)] for tau >= 0, 1 for tau < 0 (as fp32)."""
    tau = int(tau)
    return np.float32(1.0) if tau < 0 else np.float32(abar[min(tau, len(abar) - 1)])


def _coef(au, as_, at, have_hist, have_prev):
    """(c_x, c_0, c_1) in fp64 for one sample from the fp32 table values."""
    as_, at = float(as_), float(at)
    al_s, sg_s = math.sqrt(as_), math.sqrt(max(1.0 - as_, 0.0))
    al_t, sg_t = math.sqrt(at), math.sqrt(max(1.0 - at, 0.0))
    if sg_s == 0.0:
        return 0.0, 1.0, 0.0
    cx = sg_t / sg_s
    k = al_t - cx * al_s
    c0, c1 = k, 0.0
    if have_hist and have_prev and sg_t > 0.0:
        au = float(au)
        al_u, sg_u = math.sqrt(au), math.sqrt(max(1.0 - au, 0.0))

        def lam(al, sg):
            la = math.log(al) if al > 0.0 else -math.inf
            ls = math.log(sg) if sg > 0.0 else -math.inf
            return la - ls
        lu, ls, lt = lam(al_u, sg_u), lam(al_s, sg_s), lam(al_t, sg_t)
        if lu < ls < lt:
            h = lt - ls
            r = (ls - lu) / h
            c0 = k * (1.0 + 1.0 / (2.0 * r))
            c1 = -k / (2.0 * r)
    return cx, c0, c1


def coefs64(abar, t_last, t_now, t_prev):
    """fp64 coefficients [B] x 3 (abar: the fp32 table as a numpy array)."""
    abar = np.asarray(abar, dtype=np.float32)
    out = []
    for tl, tn, tp in zip(np.atleast_1d(t_last), np.atleast_1d(t_now), np.atleast_1d(t_prev)):
        ts = max(int(tn), 0)
        out.append(_coef(_abar(abar, tl) if tl >= 0 else np.float32(1.0), _abar(abar, ts), _abar(abar, tp), tl >= 0, tp >= 0))
    c = np.array(out, dtype=np.float64).reshape(-1, 3)
    return c[:, 0], c[:, 1], c[:, 2]


def coefs(abar, t_last, t_now, t_prev):
    """The kernels' coefficients: the fp64 values rounded once to fp32."""
    return tuple(c.astype(np.float32) for c in coefs64(abar, t_last, t_now, t_prev))


def _bshape(v, x):
    return np.asarray(v).reshape((-1,) + (1,) * (x.ndim - 1))


def x0_f32(x, eps, abar, t_now):
    """DDIM's fp32 x0: (x - sqrtf(fmaxf(1 - a_s, 0)) eps) / fmaxf(sqrtf(a_s), 1e-8), every operation rounded to fp32."""
    abar = np.asarray(abar, dtype=np.float32)
    a_s = np.array([_abar(abar, max(int(t), 0)) for t in np.atleast_1d(t_now)], dtype=np.float32)
    omb = np.sqrt(np.maximum(np.float32(1.0) - a_s, np.float32(0.0)))
    den = np.maximum(np.sqrt(a_s), np.float32(1e-8))
    x, eps = np.asarray(x, dtype=np.float32), np.asarray(eps, dtype=np.float32)
    return ((x - _bshape(omb, x) * eps) / _bshape(den, x)).astype(np.float32)


def step_f32(x, eps, x0_hist, abar, t_last, t_now, t_prev):
    """The fp32 mirror: returns (x_out, x0) — x0 is what the kernels leave in x0_hist."""
    x = np.asarray(x, dtype=np.float32)
    x0 = x0_f32(x, eps, abar, t_now)
    cx, c0, c1 = coefs(abar, t_last, t_now, t_prev)
    y = (_bshape(cx, x) * x + _bshape(c0, x) * x0).astype(np.float32)
    h = np.asarray(x0_hist, dtype=np.float32)
    second = _bshape(c1 != 0, x)
    y = np.where(second, y + _bshape(c1, x) * np.where(second, h, np.float32(0.0)), y).astype(np.float32)
    return y, x0


def step_f64(x, eps, x0_hist, abar, t_last, t_now, t_prev):
    """The same solver in fp64 throughout (x0 and update; coefficients unrounded).  Returns (x_out, x0)."""
    abar = np.asarray(abar, dtype=np.float32)
    x, eps = np.asarray(x, dtype=np.float64), np.asarray(eps, dtype=np.float64)
    a_s = np.array([float(_abar(abar, max(int(t), 0))) for t in np.atleast_1d(t_now)])
    x0 = (x - _bshape(np.sqrt(np.maximum(1.0 - a_s, 0.0)), x) * eps) / _bshape(np.maximum(np.sqrt(a_s), 1e-8), x)
    cx, c0, c1 = coefs64(abar, t_last, t_now, t_prev)
    y = _bshape(cx, x) * x + _bshape(c0, x) * x0
    second = _bshape(c1 != 0, x)
    h = np.where(second, np.asarray(x0_hist, dtype=np.float64), 0.0)
    return np.where(second, y + _bshape(c1, x) * h, y), x0
