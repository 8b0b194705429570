"""CPU tests of the host checks of the six whole-step slot entries (avd_denoise_step_slots_f32, _dpmpp_2m, _seeded, _guided, _cfg and
_clips): one table of refusals, every one paired with its error code and a fragment of its message, run on every entry it applies to
and on both targets.  Nothing is dereferenced before a refusal, so the descriptor is fabricated: only the ints of ``embed`` matter, and
every pointer is a non-null, 16-byte aligned stand-in.  Each row carries at least one fault, so no call reaches the model."""
import ctypes as C

import pytest

BIG = 1 << 30                                       # the stand-ins lie 1 GiB apart: far more than any buffer of these geometries
XP, TN, TP, Z, OUT, HIST, TL, WS, KNOWN, SEEDS, GSEEDS, CUR = (k * BIG for k in range(1, 13))
B, S = 2, 2
LAT = {"video": B * 8 * 4 * 16 * 16, "audio": B * 8 * 8}      # floats of z / z_out / x0_hist

ENTRIES = {      # name -> (message prefix, the riders it takes in the ABI's order, the riders it cannot do without)
    "slots": ("denoise_step_slots", (), ()),
    "dpmpp_2m": ("denoise_step_slots_dpmpp_2m", (), ("hist",)),
    "seeded": ("denoise_step_slots_seeded", ("key",), ("key",)),
    "guided": ("denoise_step_slots_guided", ("key", "guide"), ("guide",)),
    "cfg": ("denoise_step_slots_cfg", ("cfg", "key", "guide"), ("cfg",)),
    "clips": ("denoise_step_slots_clips", ("cfg", "key", "guide", "queues"), ("queues",)),
}
HIST_ENTRIES = ("dpmpp_2m", "seeded", "guided", "cfg", "clips")
KEY_ENTRIES = ("seeded", "guided", "cfg", "clips")
GUIDE_ENTRIES = ("guided", "cfg", "clips")


def _desc(target, eta=0.0, **embed):
    from multimodal_diffusion_amd import _lib as L
    d = L.StepDesc()
    e = d.embed
    e.B, e.d, e.tdim, e.Np, e.C = B, 512, 256, 10, 8
    if target == "video":
        e.target_kind, e.T, e.H, e.W, e.p0, e.p1, e.p2, e.Nt = 0, 4, 16, 16, 2, 4, 4, 32
    else:
        e.target_kind, e.T, e.H, e.W, e.p0, e.p1, e.p2, e.Nt = 1, 8, 1, 1, 4, 4, 0, 2
    for k, v in embed.items():
        setattr(e, k, v)
    d.eta = eta
    return d


def _riders(L):
    """a valid rider of every kind: key and guide share first / stride / cursor"""
    return dict(cfg=L.SlotCfg(XP, None, 0, 0.0, 0.0, None, 0), key=L.SlotKey(7, 3, S, None),
                guide=L.ClipGuide(KNOWN, None, 16, 5, 3, S, None), queues=L.ClipQueues(2, SEEDS, GSEEDS))


def _call(entry, target, *, null_desc=False, eta=0.0, embed=None, slots=S, t_last=None, hist=None, z=Z, out=OUT, **riders):
    """the entry on a fabricated descriptor; ``riders``: cfg / key / guide / queues replaced (None = a null pointer); an entry takes
    the riders of its ABI and the others are ignored.  The "dpmpp_2m" entry is given a valid history unless the row sets one."""
    from multimodal_diffusion_amd import _lib as L
    lib = L.lib()
    prefix, takes, _ = ENTRIES[entry]
    have = _riders(L)
    have.update(riders)
    if entry == "guided" and "key" not in riders and eta == 0.0:
        have["key"] = None                           # optional at eta == 0
    s = None if null_desc else C.byref(_desc(target, eta, **(embed or {})))
    rid = [None if have[r] is None else C.byref(have[r]) for r in takes]
    tail = (out, WS, 0, None)
    if entry == "slots":
        return lib.avd_denoise_step_slots_f32(s, z, XP, TN, TP, slots, *tail)
    if entry == "dpmpp_2m":
        return lib.avd_denoise_step_slots_dpmpp_2m_f32(s, z, XP, t_last, TN, TP, slots, hist, *tail)
    fn = getattr(lib, f"avd_{prefix}_f32")
    return fn(s, *rid, t_last, hist, z, XP, TN, TP, slots, *tail)


def _bad(L):
    """faulty riders by name"""
    return {"control": dict(cfg=L.SlotCfg(XP, XP, 1, 0.0, 0.0, None, 0)),                    # rescale together with APG
            "guide": dict(guide=L.ClipGuide(KNOWN, None, 0, 5, 3, S, None)),                  # P = 0
            "key": dict(key=L.SlotKey(7, 3, 0, None)),                                        # stride 0
            "key_first": dict(key=L.SlotKey(7, 4, S, None)),
            "key_stride": dict(key=L.SlotKey(7, 3, S + 1, None)),
            "key_cursor": dict(key=L.SlotKey(7, 3, S, CUR)),
            "queues": dict(queues=L.ClipQueues(3, SEEDS, GSEEDS))}                             # 3 does not divide B = 2


PAIRED = dict(t_last=TL, hist=HIST)
NOT_S = dict(slots=S + 1)


def _rows(L, entry, target):
    """(label, call keywords, code, message fragment) of every refusal that applies to ``entry``"""
    p, takes, needs = ENTRIES[entry]
    bad = _bad(L)
    base = PAIRED if entry == "dpmpp_2m" else {}      # the multistep entry cannot go without its history
    E, U = L.EINVAL, L.EUNSUPPORTED
    rows = [("null descriptor", dict(null_desc=True, **base), E, f"{p}: null descriptor")]
    null_text = {"key": "null slot key", "guide": "null clip guide", "cfg": "null slot CFG control", "queues": "null clip queues"}
    for r in needs:
        if r != "hist":
            rows.append((f"null {r}", {r: None}, E, f"{p}: {null_text[r]}"))
    if entry == "slots":
        rows.append(("eta > 0", dict(eta=0.5), E, f"{p}: slot timesteps take the DDIM update at eta == 0"))
    elif entry == "dpmpp_2m":
        rows.append(("eta > 0", dict(eta=0.5, **base), E, f"{p}: slot timesteps take the ODE update at eta == 0"))
    elif entry != "seeded":
        rows.append(("eta > 0 without a key", dict(eta=0.5, key=None), E, f"{p}: eta > 0 needs a slot key"))
    rows.append(("temb_add", dict(embed=dict(temb_add=1), **base), E, f"{p}: slot timesteps take the concat embedding (temb_add == 0)"))
    rows.append(("bad embed", dict(embed=dict(Nt=5), **base), E, "embed: token count mismatch"))
    rows.append(("bad embed widths", dict(embed=dict(d=510), **base), U, "embed: d and tdim must be multiples of 4"))
    if target == "audio":
        rows.append(("overlapping chunks", dict(embed=dict(p1=2, Nt=3), **base), U, "slot timesteps need non-overlapping audio chunks"))
    rows.append(("slots != S", dict(**NOT_S, **base), E, f"{p}: slots {S + 1} must equal the geometry's {S} slots along the sliding axis"))
    if entry in HIST_ENTRIES:
        pairing = f"{p}: null t_last or x0_hist" if entry == "dpmpp_2m" else f"{p}: t_last and x0_hist go together"
        rows.append(("t_last without x0_hist", dict(t_last=TL), E, pairing))
        rows.append(("x0_hist without t_last", dict(hist=HIST), E, pairing))
        n4 = LAT[target] * 4
        rows.append(("x0_hist aliases z", dict(t_last=TL, hist=Z + n4 - 16), E, f"{p}: x0_hist must not alias z or z_out"))
        rows.append(("x0_hist aliases z_out", dict(t_last=TL, hist=OUT - n4 + 16), E, f"{p}: x0_hist must not alias z or z_out"))
        rows.append(("misaligned x0_hist", dict(t_last=TL, hist=HIST + 4), U, f"{p}: x0_hist must be 16-byte aligned"))
    if entry in GUIDE_ENTRIES:
        rows.append(("bad guide", bad["guide"], E, "clip_guide: the clip guide's P 0 must lie in [1, 2^32]"))
        rows.append(("guide over z_out", dict(guide=L.ClipGuide(OUT + 64, None, 16, 5, 3, S, None)), E,
                     "clip_guide: known / mask must not overlap out, z_out or x0_hist"))
    if entry in KEY_ENTRIES:
        rows.append(("bad key", dict(eta=0.5, **bad["key"]), E, "slot noise: the slot key's stride must be >= 1"))
    if entry in GUIDE_ENTRIES:
        for which in ("key_first", "key_stride", "key_cursor"):
            rows.append((f"{which} differs from the guide's", dict(eta=0.5, **bad[which]), E,
                         f"{p}: the slot key's first / stride / cursor must equal the clip guide's"))
    if entry == "clips":
        rows.append(("queues do not divide B", dict(guide=None, **bad["queues"]), E, "clip_queues: the 3 queues must divide the batch 2"))
        rows.append(("queues do not divide B, guided", bad["queues"], E, "clip_guide: the 3 queues must divide the batch 2"))
        rows.append(("eta > 0 without step seeds", dict(eta=0.5, queues=L.ClipQueues(2, None, GSEEDS)), E,
                     "clip_queues: eta > 0 in a clip batch needs step_seeds"))
        rows.append(("guides without guide seeds", dict(queues=L.ClipQueues(2, SEEDS, None)), E,
                     "clip_queues: a clip guide in a clip batch needs guide_seeds"))
    # two faults at once: the first of the entry's sequence is the one reported
    order = {
        "slots": [("eta > 0 before temb_add", dict(eta=0.5, embed=dict(temb_add=1)), E, "take the DDIM update at eta == 0"),
                  ("temb_add before the embed", dict(embed=dict(temb_add=1, Nt=5)), E, "take the concat embedding"),
                  ("the embed before slots != S", dict(embed=dict(Nt=5), **NOT_S), E, "embed: token count mismatch")],
        "dpmpp_2m": [("eta > 0 before temb_add", dict(eta=0.5, embed=dict(temb_add=1), **PAIRED), E, "take the ODE update at eta == 0"),
                     ("slots != S before the pairing", dict(t_last=TL, **NOT_S), E, f"{p}: slots {S + 1} must equal"),
                     ("aliasing before alignment", dict(t_last=TL, hist=Z + 4), E, f"{p}: x0_hist must not alias z or z_out")],
        "seeded": [("the null key before temb_add", dict(key=None, embed=dict(temb_add=1)), E, f"{p}: null slot key"),
                   ("slots != S before the pairing", dict(t_last=TL, **NOT_S), E, f"{p}: slots {S + 1} must equal"),
                   ("alignment before the key", dict(eta=0.5, t_last=TL, hist=HIST + 4, **bad["key"]), U, f"{p}: x0_hist must be 16-byte aligned")],
        "guided": [("the null guide before the eta rule", dict(eta=0.5, key=None, guide=None), E, f"{p}: null clip guide"),
                   ("the pairing before the guide", dict(t_last=TL, **bad["guide"]), E, f"{p}: t_last and x0_hist go together"),
                   ("the guide before the key", dict(eta=0.5, **bad["guide"], **bad["key"]), E, "clip_guide: the clip guide's P")],
        "cfg": [("slots != S before the control", dict(**NOT_S, **bad["control"]), E, f"{p}: slots {S + 1} must equal"),
                ("the control before the pairing", dict(t_last=TL, **bad["control"]), E, "slot_cfg: guidance rescale together with APG"),
                ("alignment before the guide", dict(t_last=TL, hist=HIST + 4, **bad["guide"]), U, f"{p}: x0_hist must be 16-byte aligned"),
                ("the key before the geometry", dict(eta=0.5, key=L.SlotKey(7, 4, 0, None)), E, "slot noise: the slot key's stride")],
        "clips": [("the null queues before the eta rule", dict(eta=0.5, key=None, queues=None), E, f"{p}: null clip queues"),
                  ("the control before the pairing", dict(hist=HIST, **bad["control"]), E, "slot_cfg: guidance rescale together with APG"),
                  ("the guide before the key", dict(eta=0.5, **bad["guide"], **bad["key"]), E, "clip_guide: the clip guide's P"),
                  ("the geometry before the queues", dict(eta=0.5, queues=L.ClipQueues(2, None, GSEEDS), **bad["key_first"]), E,
                   f"{p}: the slot key's first / stride / cursor must equal")],
    }
    return rows + order[entry]


@pytest.mark.parametrize("target", ["video", "audio"])
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_slot_step_entries_refuse_before_the_model_runs(entry, target):
    from multimodal_diffusion_amd import _lib as L
    lib = L.lib()
    rows = _rows(L, entry, target)
    assert len(rows) >= 9
    for label, kw, code, fragment in rows:
        rc = _call(entry, target, **kw)
        err = lib.avd_last_error().decode()
        assert rc == code and fragment in err, (entry, target, label, rc, err)

