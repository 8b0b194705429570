"""References of the slot-timestep tests ("slot timesteps" in include/avdiff_hip.h), built from the CPU oracle's parts and from plain
torch, without the code under test: the [B, S] timestep tables of the tests, the per-pair composition the bit-exact tests compare
against, the oracle's whole step with one timestep per slot, and the torch restatement of the FIFO queue shift."""
import torch

from oracle import ref_cpu as R

SCHED = R.sampling_schedule(1000, 20).tolist()          # a 1000-step table sampled in 20 steps: 999, 949, ..., 49, -1


def tables(B, S, seed=0):
    """Random [B, S] tables (CPU int64) drawn from SCHED: every slot a pair (s_i, s_{i+1}) or a hold (t_prev == t_now); the tables
    hold a final step (t_prev = -1) and a hold, and every sample with S >= 2 holds two distinct pairs."""
    g = torch.Generator().manual_seed(seed)
    i = torch.randint(0, len(SCHED) - 1, (B, S), generator=g)
    sc = torch.tensor(SCHED)
    tn, tp = sc[i], sc[i + 1]
    for b in range(B):
        if S >= 2 and i[b, 0] == i[b, 1]:
            j = (int(i[b, 0]) + 1) % (len(SCHED) - 1)
            tn[b, 1], tp[b, 1] = sc[j], sc[j + 1]
    tn[0, S - 1], tp[0, S - 1] = sc[-2], sc[-1]           # the final step of a trajectory
    tp[B - 1, 0] = tn[B - 1, 0]                           # a hold
    assert (tp == -1).any() and (tp == tn).any()
    assert all(len({(int(a), int(p)) for a, p in zip(tn[b], tp[b])}) >= min(S, 2) for b in range(B))
    return tn.contiguous(), tp.contiguous()


def slot_of_position(L_, slot_len, S):
    """the slot of every position of the sliding axis: l // slot_len, the uncovered tail following the last slot"""
    return torch.clamp(torch.arange(L_) // slot_len, max=S - 1)


def per_position(t, L_, slot_len, z):
    """a [B, S] table -> the timestep of every element of z ([B, C, L, ...]), broadcastable to z"""
    B, S = t.shape
    tl = t[:, slot_of_position(L_, slot_len, S).to(t.device)]
    return tl.view((B, 1, L_) + (1,) * (z.dim() - 3))


def by_pairs(per_sample, z, tn, tp, slot_len):
    """The reference of the bit-exact tests: ``per_sample(t_now [B], t_prev [B])`` (the existing per-sample entry, on uniform
    timesteps) is called once per distinct pair of the tables and its output kept on that pair's slots; held slots are z."""
    B = z.shape[0]
    L_ = z.shape[2]
    tn_e, tp_e = per_position(tn.to(z.device), L_, slot_len, z), per_position(tp.to(z.device), L_, slot_len, z)
    out = z.clone()
    for a, p in sorted({(int(a), int(p)) for a, p in zip(tn.reshape(-1).tolist(), tp.reshape(-1).tolist())}):
        if a == p:
            continue
        full = per_sample(torch.full((B,), a, dtype=torch.long, device=z.device), torch.full((B,), p, dtype=torch.long, device=z.device))
        out = torch.where((tn_e == a) & (tp_e == p), full, out)
    return out


def ddim_slots(z, eps_lat, tn, tp, slot_len):
    """the oracle's DDIM update with one pair per slot: every sliding position is a row of R.ddim_update; held slots are z"""
    B, L_ = z.shape[0], z.shape[2]
    S = tn.shape[1]
    sl = slot_of_position(L_, slot_len, S)
    rows = lambda x: x.movedim(2, 1).reshape((B * L_,) + tuple(x.shape[1:2]) + tuple(x.shape[3:]))
    out = R.ddim_update(rows(z), tn[:, sl].reshape(-1), tp[:, sl].reshape(-1), rows(eps_lat), R.alpha_bar_table(R.beta_table(1000)))
    out = out.view((B, L_) + tuple(z.shape[1:2]) + tuple(z.shape[3:])).movedim(1, 2)
    hold = per_position(tn, L_, slot_len, z) == per_position(tp, L_, slot_len, z)
    return torch.where(hold, z, out)


def step_slots(ws, target, z, zp, tn, tp, guidance, tube=(2, 4, 4), chunk=(4, 4), tdim=256):
    """The oracle composition of one step on slot timesteps (CPU tensors): per-token R.timestep_embedding, R.eps_pair, the CFG
    combine, un-patch / overlap-add and the per-slot DDIM update."""
    B = z.shape[0]
    S = tn.shape[1]
    if target == "video":
        _, C, T, H, W = z.shape
        tok, tokp = R.tube_patch(z, *tube), R.audio_tokens(zp, *chunk)
        at, ap = ws["adapt_v"], ws["adapt_a"]
        per_slot = tok.shape[1] // S
    else:
        _, Ca, F = z.shape
        tok, tokp = R.audio_tokens(z, *chunk), R.tube_patch(zp, *tube)
        at, ap = ws["adapt_a"], ws["adapt_v"]
        per_slot = 1
    slot = torch.arange(tok.shape[1]) // per_slot
    x = R.linear(tok, at["proj.weight"], at["proj.bias"])
    e = R.timestep_embedding(tn[:, slot].reshape(-1), tdim).view(B, tok.shape[1], tdim)
    Xt = torch.cat([x, e], -1)
    Xp = R.embed_with_time(tokp, ap["proj.weight"], ap["proj.bias"], torch.zeros(B, dtype=torch.long), tdim)
    e_c, e_n = R.eps_pair(Xt, Xp, target == "video", ws["core"], ws["head"], target, 2, 8)
    eps_tok = e_n + guidance * (e_c - e_n)
    if target == "video":
        return ddim_slots(z, R.tube_unpatch(eps_tok, C, T, H, W, *tube), tn, tp, tube[0])
    return ddim_slots(z, R.audio_untokens(eps_tok, Ca, chunk[0], F, chunk[1]), tn, tp, chunk[0])


def shift(z, tail, slot_len):
    """The queue shift in torch: the batch [B, C, L, ...] as a queue of B * S slots along L, rolled by one slot towards the head;
    ``tail`` ([C, slot_len, ...]) fills the last slot.  Returns (z_out, popped)."""
    B, L_ = z.shape[0], z.shape[2]
    S = L_ // slot_len
    q = z.movedim(2, 1).reshape((B * S, slot_len) + tuple(z.shape[1:2]) + tuple(z.shape[3:]))      # [queue slot, j, C, ...]
    popped = q[0].movedim(0, 1).contiguous()
    q = torch.roll(q, -1, 0)
    q[-1] = tail.movedim(1, 0)
    out = q.view((B, L_) + tuple(z.shape[1:2]) + tuple(z.shape[3:])).movedim(1, 2).contiguous()
    return out, popped
