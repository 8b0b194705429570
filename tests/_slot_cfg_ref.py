"""numpy mirror of the slot CFG control (include/avdiff_hip.h, "slot CFG control"), built from the per-sample mirrors _cfg_ref and
_apg_ref applied to one slot at a time: the level lookup, the combine in fp32, the per-slot rescale factor / APG coefficients from fp64
moments, and the controlled eps tokens.  Shared by tests/test_slot_cfg_cpu.py and tests/test_gpu_slot_cfg.py."""
import numpy as np

import _apg_ref as AR
import _cfg_ref as CR

F32 = np.float32
NEUTRAL = np.array([1.0, 0.0, 0.0, 0.0], F32)        # what the finalize pass stores for a held slot


def level(t_now, T_train):
    """i = min(max(t_now, 0), T_train - 1)"""
    return np.clip(np.asarray(t_now, np.int64), 0, T_train - 1)


def slot_tokens(tok, S):
    """tokens [B, Nt, D] -> [B, S, Nt / S * D]: slot s is the Nt / S consecutive tokens s * Nt / S .. (video: t' = s; audio: token s)"""
    tok = np.asarray(tok, F32)
    B, Nt, D = tok.shape
    assert Nt % S == 0
    return tok.reshape(B, S, (Nt // S) * D)


def apply(cond_tok, null_tok, coef, apg):
    """the controlled eps tokens [B, Nt, D] from given per-slot coefficients [B, S, 4] (the scratch's layout): elementwise and exact,
    r(null + g (cond - null)) with (s, g, phi, 0), or cond + w (d - k cond) with (s, k, w, g)"""
    coef = np.asarray(coef, F32)
    B, S = coef.shape[:2]
    c, u = slot_tokens(cond_tok, S).reshape(B * S, -1), slot_tokens(null_tok, S).reshape(B * S, -1)
    q = coef.reshape(B * S, 4)
    if apg:
        e = AR.combine_f32(c, AR.direction(c, u), q[:, 2], q[:, 1])
    else:
        e = CR.rescale_f32(CR.combine_f32(c, u, q[:, 1]), q[:, 2], q[:, 0])
    return e.reshape(np.shape(cond_tok))


def control(cond_tok, null_tok, t_now, t_prev, guidance, T_train, guidance_t=None, rescale_t=None, apg=None):
    """(eps tokens [B, Nt, D] fp32, coef [B, S, 4] fp32): the eps every stepping slot steps on and the four floats the scratch holds
    per slot — (s, g, phi, 0) under a rescale (also returned, with s = 1, for a guidance table alone, which has no scratch),
    (s, k, w, g) under ``apg`` = (r, eta_p); NEUTRAL for a held slot, whose eps tokens are returned as the plain combine and are not
    read by anyone.  ``t_now`` / ``t_prev``: int [B, S]."""
    assert apg is None or rescale_t is None
    tn, tp = np.asarray(t_now, np.int64), np.asarray(t_prev, np.int64)
    B, S = tn.shape
    shape = np.shape(cond_tok)
    c_all, u_all = slot_tokens(cond_tok, S), slot_tokens(null_tok, S)
    out = np.empty_like(c_all)
    coef = np.empty((B, S, 4), F32)
    lv = level(tn, T_train)
    for b in range(B):
        for s in range(S):
            c, u = c_all[b, s][None], u_all[b, s][None]          # one "sample" of the per-sample mirrors
            if tn[b, s] == tp[b, s]:
                out[b, s], coef[b, s] = CR.combine_f32(c, u, guidance)[0], NEUTRAL
                continue
            g = F32(guidance) if guidance_t is None else F32(np.asarray(guidance_t, F32)[lv[b, s]])
            phi = F32(0.0) if rescale_t is None else F32(np.asarray(rescale_t, F32)[lv[b, s]])
            if apg is not None:
                e, _, (sb, kb, wb) = AR.apg(c, u, g, apg[0], apg[1])
                out[b, s], coef[b, s] = e[0], (sb[0], kb[0], wb[0], g)
            else:
                y = CR.combine_f32(c, u, g)
                sb = CR.scale(c, y) if rescale_t is not None else np.ones(1, F32)
                out[b, s], coef[b, s] = CR.rescale_f32(y, phi, sb)[0], (sb[0], g, phi, 0.0)
    return out.reshape(shape), coef
