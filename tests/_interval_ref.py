"""numpy mirror of the cond-only step of a guidance interval (contract in include/avdiff_hip.h, "guidance interval"), and the
reference trajectory under an interval.

``cond_update_f64``: eps = eps_cond exactly, then the solver's update in fp64 — DDIM (eta, explicit noise) written out here, or
DPM-Solver++(2M) — and nothing else: no null branch, no combine, no rescale.
"""
import numpy as np


def _a(abar, tau):
    tau = int(tau)
    return 1.0 if tau < 0 else float(np.float32(abar[min(tau, len(abar) - 1)]))


def _b(v, x):
    return np.asarray(v, dtype=np.float64).reshape((-1,) + (1,) * (x.ndim - 1))


def cond_update_f64(x, eps_cond, abar, t_now, t_prev, *, eta=0.0, noise=None, solver="ddim", x0_hist=None, t_last=None):
    """(z_out, x0): one cond-only update in fp64 on latent-layout eps_cond."""
    x, e = np.asarray(x, dtype=np.float64), np.asarray(eps_cond, dtype=np.float64)
    a_t = np.array([_a(abar, max(int(t), 0)) for t in t_now])
    a_p = np.array([_a(abar, t) for t in t_prev])
    x0 = (x - _b(np.sqrt(np.maximum(1.0 - a_t, 0.0)), x) * e) / _b(np.maximum(np.sqrt(a_t), 1e-8), x)
    if solver == "dpmpp_2m":
        import _dpm_ref as D
        cx, c0, c1 = D.coefs64(abar, t_last, t_now, t_prev)
        second = _b(c1 != 0, x).astype(bool)
        h = np.where(second, np.asarray(x0_hist, dtype=np.float64), 0.0)
        y = _b(cx, x) * x + _b(c0, x) * x0
        return np.where(second, y + _b(c1, x) * h, y), x0
    sigma = np.zeros_like(a_t)
    if eta > 0:
        frac = np.maximum((1.0 - a_p) / np.maximum(1.0 - a_t, 1e-8), 0.0)
        omr = np.maximum(1.0 - a_t / np.maximum(a_p, 1e-8), 0.0)
        sigma = eta * np.sqrt(frac * omr)
    c_eps = np.sqrt(np.maximum(1.0 - a_p - sigma ** 2, 0.0))
    zn = 0.0 if noise is None else np.asarray(noise, dtype=np.float64)
    return _b(np.sqrt(a_p), x) * x0 + _b(c_eps, x) * e + _b(sigma, x) * zn, x0


def step_kinds(sched, interval):
    """[cfg?] per step of the schedule, written without the function under test: t_lo <= sched[i] <= t_hi."""
    s = [int(t) for t in np.asarray(sched).reshape(-1)]
    return [interval is None or interval[0] <= t <= interval[1] for t in s[:-1]]
