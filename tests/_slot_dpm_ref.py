"""References of the slot form of DPM-Solver++(2M) ("slot timesteps" in include/avdiff_hip.h), built from the numpy mirror of the
solver (_dpm_ref), the slot references (_slot_ref) and the CPU oracle's parts, without the code under test: the [B, S] triple tables of
the tests, the per-triple composition the bit-exact tests compare against, the per-slot numpy mirror in fp32 and fp64, and the oracle's
whole step with one timestep per slot ending in the solver's update."""
import numpy as np
import torch

import _dpm_ref as D
import _slot_ref as SR
from oracle import ref_cpu as R

SCHED = SR.SCHED
ABAR = R.alpha_bar_table(R.beta_table(1000)).numpy()


def tables3(B, S, seed=0):
    """Random [B, S] tables (t_last, t_now, t_prev), CPU int64, drawn from SCHED = s_0 > ... > s_n = -1.  Every slot starts as a genuine
    second-order triple (s_{i-1}, s_i, s_{i+1}); then one slot each becomes a final step (t_prev = -1), a hold (t_prev == t_now), a
    mis-ordered history (t_last <= t_now: first order by the lambda condition) and a first-order triple (t_last = -1).  With only four
    slots (B = S = 2) the final step carries the t_last = -1: a final step is first order whatever its history, so nothing is lost.
    Every sample then holds two distinct triples."""
    assert B >= 2 and S >= 2, "the special slots need their own positions"
    n = len(SCHED) - 1
    g = torch.Generator().manual_seed(seed)
    i = torch.randint(1, n - 1, (B, S), generator=g)          # s_{i+1} >= s_{n-1} >= 0: not a final step
    for b in range(B):
        if i[b, 0] == i[b, 1]:
            i[b, 1] = i[b, 0] % (n - 2) + 1
    sc = torch.tensor(SCHED)
    tl, tn, tp = sc[i - 1].clone(), sc[i].clone(), sc[i + 1].clone()
    tl[0, S - 1], tn[0, S - 1], tp[0, S - 1] = sc[n - 2], sc[n - 1], sc[n]          # the final step of a trajectory, with a history
    tp[B - 1, 0] = tn[B - 1, 0]                                                     # a hold
    tl[B - 1, S - 1] = tp[B - 1, S - 1]                                             # a history below t_now
    free = [(b, s) for b in range(B) for s in range(S) if (b, s) not in ((0, S - 1), (B - 1, 0), (B - 1, S - 1))]
    if len(free) >= 2:
        tl[free[-1]] = -1                                                           # no history
    else:
        tl[0, S - 1] = -1
    hold = tp == tn
    second = (tl > tn) & (tp >= 0) & ~hold
    assert ((tl == -1) & ~hold).any(), "a first-order triple (t_last = -1)"
    runs = set(zip(SCHED[:-2], SCHED[1:-1], SCHED[2:]))
    assert second.any() and all((int(a), int(b), int(c)) in runs for a, b, c in zip(tl[second], tn[second], tp[second])), \
        "a genuine second-order triple"
    assert (tp == -1).any(), "a final step"
    assert hold.any(), "a hold"
    assert ((tl >= 0) & (tl <= tn) & ~hold & (tp >= 0)).any(), "a mis-ordered history"
    assert all(len({(int(u), int(a), int(p)) for u, a, p in zip(tl[b], tn[b], tp[b])}) >= 2 for b in range(B))
    return tl.contiguous(), tn.contiguous(), tp.contiguous()


def by_triples(per_sample, z, h, tl, tn, tp, slot_len):
    """As _slot_ref.by_pairs, returning the history as well: ``per_sample(t_last [B], t_now [B], t_prev [B])`` -> (z_out, x0_hist), the
    per-sample entry on uniform timesteps started from the history ``h``, is called once per distinct triple of the tables and both
    outputs kept on that triple's slots; held slots are (z, h)."""
    B, L_ = z.shape[0], z.shape[2]
    el = [SR.per_position(t.to(z.device), L_, slot_len, z) for t in (tl, tn, tp)]
    out, hist = z.clone(), h.clone()
    for u, a, p in sorted(set(zip(tl.reshape(-1).tolist(), tn.reshape(-1).tolist(), tp.reshape(-1).tolist()))):
        if a == p:
            continue
        full, fh = per_sample(*(torch.full((B,), v, dtype=torch.long, device=z.device) for v in (u, a, p)))
        on = (el[0] == u) & (el[1] == a) & (el[2] == p)
        out, hist = torch.where(on, full, out), torch.where(on, fh, hist)
    return out, hist


def step_slots_np(step, z, eps, h, tl, tn, tp, slot_len):
    """The per-slot mirror: ``step`` (_dpm_ref.step_f32 or step_f64) applied per sliding position — every position of z, eps and h
    ([B, C, L, ...] numpy arrays) is one row of the per-sample reference, with the triple of its slot; held slots keep (z, h).
    Returns (z_out, x0_hist) in the dtype ``step`` works in."""
    z, eps, h = (np.asarray(a) for a in (z, eps, h))
    B, L_ = z.shape[0], z.shape[2]
    sl = SR.slot_of_position(L_, slot_len, tn.shape[1]).numpy()
    rows = lambda x: np.moveaxis(x, 2, 1).reshape((B * L_,) + x.shape[1:2] + x.shape[3:])
    back = lambda x: np.moveaxis(x.reshape((B, L_) + z.shape[1:2] + z.shape[3:]), 1, 2)
    u, a, p = (np.asarray(t)[:, sl].reshape(-1) for t in (tl, tn, tp))
    out, x0 = step(rows(z), rows(eps), rows(h), ABAR, u, a, p)
    hold = back(np.broadcast_to((a == p).reshape((-1,) + (1,) * (z.ndim - 2)), rows(z).shape))
    return np.where(hold, z.astype(out.dtype), back(out)), np.where(hold, h.astype(x0.dtype), back(x0))


def mirror_slots(z, eps, h, tl, tn, tp, slot_len):
    """the fp32 mirror of the slot update on torch CPU tensors -> (z_out, x0_hist) as torch tensors"""
    out, x0 = step_slots_np(D.step_f32, z.numpy(), eps.numpy(), h.numpy(), tl, tn, tp, slot_len)
    return torch.from_numpy(np.ascontiguousarray(out)), torch.from_numpy(np.ascontiguousarray(x0))


def oracle_eps(ws, target, z, zp, tn, guidance, tube=(2, 4, 4), chunk=(4, 4), tdim=256):
    """The oracle's guided eps latent of one step on slot timesteps (CPU tensors): the front of _slot_ref.step_slots — per-token
    R.timestep_embedding, R.eps_pair, the CFG combine, un-patch / overlap-add — without its DDIM update."""
    B, S = z.shape[0], tn.shape[1]
    if target == "video":
        tok, tokp = R.tube_patch(z, *tube), R.audio_tokens(zp, *chunk)
        at, ap = ws["adapt_v"], ws["adapt_a"]
        per_slot = tok.shape[1] // S
    else:
        tok, tokp = R.audio_tokens(z, *chunk), R.tube_patch(zp, *tube)
        at, ap = ws["adapt_a"], ws["adapt_v"]
        per_slot = 1
    slot = torch.arange(tok.shape[1]) // per_slot
    x = R.linear(tok, at["proj.weight"], at["proj.bias"])
    e = R.timestep_embedding(tn[:, slot].reshape(-1), tdim).view(B, tok.shape[1], tdim)
    Xp = R.embed_with_time(tokp, ap["proj.weight"], ap["proj.bias"], torch.zeros(B, dtype=torch.long), tdim)
    e_c, e_n = R.eps_pair(torch.cat([x, e], -1), Xp, target == "video", ws["core"], ws["head"], target, 2, 8)
    eps_tok = e_n + guidance * (e_c - e_n)
    if target == "video":
        return R.tube_unpatch(eps_tok, *z.shape[1:], *tube)
    return R.audio_untokens(eps_tok, z.shape[1], chunk[0], z.shape[2], chunk[1])


def oracle_step_slots(ws, target, z, zp, h, tl, tn, tp, guidance, slot_len):
    """the oracle's whole step on slot timesteps ending in the fp64 solver update per slot -> (z_out, x0_hist), float64 tensors"""
    eps = oracle_eps(ws, target, z, zp, tn, guidance)
    out, x0 = step_slots_np(D.step_f64, z.numpy(), eps.numpy(), h.numpy(), tl, tn, tp, slot_len)
    return torch.from_numpy(np.ascontiguousarray(out)), torch.from_numpy(np.ascontiguousarray(x0))
