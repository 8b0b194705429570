"""References of the FIFO lookahead tests ("FIFO lookahead" in include/avdiff_hip.h), in plain torch and Python, without the code under
test: the logical-queue map (owner lookup, shift, duplicates), the plan rows written out from their definitions, the prompt windows
of the overlapping queue, and the driver loop built from parts the caller hands in."""
import torch


# ------------------------------------------------------------------------------------------------- the logical-queue map
def owner(q, S, ctx):
    """(window, slot) of the owner copy of logical slot q: the context in window 0, active slot a in window a // h at ctx + a % h"""
    h = S - ctx
    return (0, q) if q < ctx else ((q - ctx) // h, ctx + (q - ctx) % h)


def slot(z, k, s, slot_len):
    """window k, slot s of a batch [B, C, L, ...]: [C, slot_len, ...]"""
    return z[k][:, s * slot_len:(s + 1) * slot_len]


def logical(z, ctx, slot_len):
    """Old[0 .. Q-1]: the owner copy of every logical slot of the batch z"""
    B, S = z.shape[0], z.shape[2] // slot_len
    return [slot(z, *owner(q, S, ctx), slot_len) for q in range(ctx + B * (S - ctx))]


def windows(old, B, S, ctx, first=0):
    """the batch whose window k slot s is old[k*h + s + first]"""
    h = S - ctx
    return torch.stack([torch.cat([old[k * h + s + first] for s in range(S)], 1) for k in range(B)], 0).contiguous()


def lookahead(z, ctx, shift, slot_len, tail=None):
    """(z_out, popped) of the lookahead launch: z_out window k slot s = Old[k*h + s + shift] with Old[Q] = ``tail``; popped = Old[ctx]
    at shift 1, None at shift 0"""
    B, S = z.shape[0], z.shape[2] // slot_len
    old = logical(z, ctx, slot_len)
    if shift:
        old = old + [tail]
    return windows(old, B, S, ctx, shift), (old[ctx].clone() if shift else None)


def lookahead_hist(hist, ctx, shift, slot_len):
    """hist_out: the same map on the stepping positions, zeros in the entering tail and on every context position"""
    out, _ = lookahead(hist, ctx, shift, slot_len, torch.zeros_like(slot(hist, 0, 0, slot_len)))
    out[:, :, :ctx * slot_len] = 0
    return out


def coherent(z, ctx, slot_len):
    """every copy of a logical slot equals its owner"""
    B, S = z.shape[0], z.shape[2] // slot_len
    old = logical(z, ctx, slot_len)
    return all(torch.equal(slot(z, k, s, slot_len), old[k * (S - ctx) + s]) for k in range(B) for s in range(S))


# ------------------------------------------------------------------------------------------------- the plan
def _ramp_slot(s, n, ctx, context, r, q):
    """(t_now, t_prev, t_last) of logical slot q in ramp iteration r"""
    if q < ctx:
        lab = s[0] if context == "noise" else 0
        return lab, lab, -1
    a = q - ctx
    if a > r:
        return s[0], s[0], -1
    i = r - a
    return s[i], s[i + 1], (s[i - 1] if i else -1)


def _steady_slot(s, n, ctx, context, row, q):
    """(t_now, t_prev, t_last) of logical slot q in the steady row `row` = min(m, ctx)"""
    if q < ctx:
        lab = 0 if (context == "clean" or q >= ctx - row) else s[0]
        return lab, lab, -1
    i = n - 1 - (q - ctx)
    return s[i], s[i + 1], (s[i - 1] if i else -1)


def plan(sched, S, ctx, context="noise"):
    """(ramp_now, ramp_prev, ramp_last [n-1, B, S], steady_now, steady_prev, steady_last [ctx+1, B, S]) from the definitions: window k
    position p holds logical slot k*h + p; p >= ctx takes its slot's triple, p < ctx is held at its slot's t_now with t_last -1"""
    s = [int(v) for v in sched]
    n, h = len(s) - 1, S - ctx
    B = n // h

    def rows(n_rows, f):
        t = torch.empty(3, n_rows, B, S, dtype=torch.long)
        for r in range(n_rows):
            for k in range(B):
                for p in range(S):
                    now, prev, last = f(s, n, ctx, context, r, k * h + p)
                    t[:, r, k, p] = torch.tensor([now, prev, last] if p >= ctx else [now, now, -1])
        return t[0], t[1], t[2]

    return rows(n - 1, _ramp_slot) + rows(ctx + 1, _steady_slot)


# ------------------------------------------------------------------------------------------------- the driver
def prompt_windows(canvas, first, B, stride, hop, Lp):
    """window k = prompt positions (first + k*stride)*hop .. + Lp - 1 of the canvas's axis 1, zeros outside the canvas"""
    P = canvas.shape[1]
    out = canvas.new_zeros((B, canvas.shape[0], Lp) + tuple(canvas.shape[2:]))
    for k in range(B):
        for l in range(Lp):
            p = (first + k * stride) * hop + l
            if 0 <= p < P:
                out[k, :, l] = canvas[:, p]
    return out


def loop(eng, canvas_p, hop, Lp, sched, K, ctx, canvas_noise, context=None):
    """fifo_denoise(lookahead=ctx) restated from its parts: the plan rows above, eng.step_slots, the torch map, eng.set_prompt with the
    shifted prompt windows.  ``canvas_noise(positions0, n_pos)`` -> [C, n_pos, ...]: the seeded normals at s_0 of canvas positions
    positions0 .. positions0 + n_pos - 1 (modulo 2^32).  On solver "dpmpp_2m" the history follows ``lookahead_hist``."""
    B, S, sl = eng.embed.B, eng.slots, eng.slot_len
    h = S - ctx
    n = B * h
    rn, rp, rl, sn, sp, slast = plan(sched, S, ctx, "noise" if context is None else "clean")
    dpm = eng.solver == "dpmpp_2m"
    head = canvas_noise(2 ** 32 - ctx * sl, ctx * sl) if context is None else context
    act = canvas_noise(0, n * sl)
    old = [head[:, q * sl:(q + 1) * sl] for q in range(ctx)] + [act[:, a * sl:(a + 1) * sl] for a in range(n)]
    z = windows(old, B, S, ctx)
    eng.set_prompt(prompt_windows(canvas_p, -ctx, B, h, hop, Lp))
    for r in range(n - 1):
        z = eng.step_slots(z, rn[r], rp[r], t_last=rl[r] if dpm else None)
        if dpm:
            eng.x0_hist.copy_(lookahead_hist(eng.x0_hist, ctx, 0, sl))
        z, _ = lookahead(z, ctx, 0, sl)
    done = []
    for m in range(K):
        eng.set_prompt(prompt_windows(canvas_p, m - ctx, B, h, hop, Lp))
        row = min(m, ctx)
        z = eng.step_slots(z, sn[row], sp[row], t_last=slast[row] if dpm else None)
        if dpm:
            eng.x0_hist.copy_(lookahead_hist(eng.x0_hist, ctx, 1, sl))
        z, popped = lookahead(z, ctx, 1, sl, canvas_noise((n + m) * sl, sl))
        done.append(popped)
    return torch.cat(done, 1)
