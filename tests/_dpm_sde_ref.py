"""numpy reference of the SDE-DPM-Solver++(2M) update (contract in include/avdiff_hip.h, avd_dpmpp_2m_sde_step_f32): the ODE
reference of _dpm_ref.py with an ``eta`` and a noise term.

  * ``coefs64`` / ``coefs``: (c_x, c_0, c_1, c_n) per sample, in fp64 from the fp32 table / rounded once to fp32.  eta == 0 evaluates
    the ODE expressions of _dpm_ref (c_n = 0), as the kernels do;
  * ``step_f32``: the fp32 mirror of the kernels — x0 with DDIM's fp32 expression, the update in fp32 in the contract's order
    ((c_x x + c_0 x0) [+ c_1 hist]) + c_n n, every operation rounded, the noise term only at eta > 0;
  * ``step_f64``: the same solver in plain fp64.
The normals are not drawn here: tests take them from _noise_ref / _canvas_noise_ref or from the device stream."""
import math

import numpy as np

import _dpm_ref as D
from _dpm_ref import _abar, _bshape, x0_f32  # noqa: F401  (x0_f32 is part of this module's interface)


def _lam(al, sg):
    la = math.log(al) if al > 0.0 else -math.inf
    ls = math.log(sg) if sg > 0.0 else -math.inf
    return la - ls


def _coef(au, as_, at, have_hist, have_prev, eta):
    """(c_x, c_0, c_1, c_n) in fp64 for one sample from the fp32 table values, eta > 0."""
    as_, at = float(as_), float(at)
    al_s, sg_s = math.sqrt(as_), math.sqrt(max(1.0 - as_, 0.0))
    al_t, sg_t = math.sqrt(at), math.sqrt(max(1.0 - at, 0.0))
    if sg_s == 0.0:
        return 0.0, 1.0, 0.0, 0.0
    if sg_t == 0.0:                                  # h = +inf: x0_s, no noise
        return 0.0, al_t, 0.0, 0.0
    ls, lt = _lam(al_s, sg_s), _lam(al_t, sg_t)
    h = lt - ls
    cx = (sg_t / sg_s) * math.exp(-eta * h)
    k = al_t * (-math.expm1(-(1.0 + eta) * h))
    cn = sg_t * math.sqrt(max(-math.expm1(-2.0 * eta * h), 0.0))
    c0, c1 = k, 0.0
    if have_hist and have_prev:
        au = float(au)
        lu = _lam(math.sqrt(au), math.sqrt(max(1.0 - au, 0.0)))
        if lu < ls < lt:
            r = (ls - lu) / h
            c0 = k * (1.0 + 1.0 / (2.0 * r))
            c1 = -k / (2.0 * r)
    return cx, c0, c1, cn


def coefs64(abar, t_last, t_now, t_prev, eta):
    """fp64 coefficients [B] x 4 (abar: the fp32 table as a numpy array)."""
    eta = float(np.float32(eta))                     # the kernels receive eta as fp32
    if eta == 0.0:
        cx, c0, c1 = D.coefs64(abar, t_last, t_now, t_prev)
        return cx, c0, c1, np.zeros_like(cx)
    abar = np.asarray(abar, dtype=np.float32)
    out = []
    for tl, tn, tp in zip(np.atleast_1d(t_last), np.atleast_1d(t_now), np.atleast_1d(t_prev)):
        ts = max(int(tn), 0)
        out.append(_coef(_abar(abar, tl) if tl >= 0 else np.float32(1.0), _abar(abar, ts), _abar(abar, tp), tl >= 0, tp >= 0, eta))
    c = np.array(out, dtype=np.float64).reshape(-1, 4)
    return c[:, 0], c[:, 1], c[:, 2], c[:, 3]


def coefs(abar, t_last, t_now, t_prev, eta):
    """The kernels' coefficients: the fp64 values rounded once to fp32."""
    return tuple(c.astype(np.float32) for c in coefs64(abar, t_last, t_now, t_prev, eta))


def step_f32(x, eps, x0_hist, abar, t_last, t_now, t_prev, eta, noise=None):
    """The fp32 mirror: returns (x_out, x0) — x0 is what the kernels leave in x0_hist.  ``noise`` is read at eta > 0 only."""
    x = np.asarray(x, dtype=np.float32)
    x0 = x0_f32(x, eps, abar, t_now)
    cx, c0, c1, cn = coefs(abar, t_last, t_now, t_prev, eta)
    y = (_bshape(cx, x) * x + _bshape(c0, x) * x0).astype(np.float32)
    h = np.asarray(x0_hist, dtype=np.float32)
    second = _bshape(c1 != 0, x)
    y = np.where(second, y + _bshape(c1, x) * np.where(second, h, np.float32(0.0)), y).astype(np.float32)
    if eta > 0:
        y = (y + (_bshape(cn, x) * np.asarray(noise, dtype=np.float32)).astype(np.float32)).astype(np.float32)
    return y, x0


def step_f64(x, eps, x0_hist, abar, t_last, t_now, t_prev, eta, noise=None, second_order=True):
    """The same solver in fp64 throughout (x0 and update; coefficients unrounded).  Returns (x_out, x0).  ``second_order=False``
    switches the history off (the first-order SDE solver, for the order-of-convergence check)."""
    abar = np.asarray(abar, dtype=np.float32)
    x, eps = np.asarray(x, dtype=np.float64), np.asarray(eps, dtype=np.float64)
    a_s = np.array([float(_abar(abar, max(int(t), 0))) for t in np.atleast_1d(t_now)])
    x0 = (x - _bshape(np.sqrt(np.maximum(1.0 - a_s, 0.0)), x) * eps) / _bshape(np.maximum(np.sqrt(a_s), 1e-8), x)
    if not second_order:
        t_last = np.full(np.atleast_1d(t_now).shape, -1)
    cx, c0, c1, cn = coefs64(abar, t_last, t_now, t_prev, eta)
    y = _bshape(cx, x) * x + _bshape(c0, x) * x0
    second = _bshape(c1 != 0, x)
    h = np.where(second, np.asarray(x0_hist, dtype=np.float64), 0.0)
    y = np.where(second, y + _bshape(c1, x) * h, y)
    if eta > 0:
        y = y + _bshape(cn, x) * np.asarray(noise, dtype=np.float64)
    return y, x0
