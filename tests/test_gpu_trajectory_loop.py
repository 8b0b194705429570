"""DenoiseEngine.run on the MI355X at the short trajectories where the branches of its one loop meet (1 .. 5 steps, and an 8-step
guidance interval): the result against a hand-driven chain of ``step`` calls, bit for bit, and the sequence of host events — E an
eager ``advance``, C a ``capture_pair``, R a replay — against the sequence the loop is specified to take (capture and replay
enqueue no step of their own, so the sequence is what the run costs)."""
import pytest
import torch

from _kit import audio_case, dev, engine, model, ts, video_case  # noqa: F401  (dev / model are fixtures)
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
G = 3.0
EAGER = {n: "E" * n for n in range(1, 6)}
GRAPH = {1: "E", 2: "EE", 3: "ECR", 4: "ECRE", 5: "ECRR"}         # warm-up step, one captured pair, its replays, the odd tail


class Events:
    """the host events of an engine's runs: "E" / "C" / "R" with the kind of step attached (f: full CFG, c: cond-only); the two
    advances inside a capture belong to its "C" """

    def __init__(self, eng, monkeypatch):
        from multimodal_diffusion_amd import sampler
        self.log, self._capturing, self._kind = [], False, {}
        advance, capture_pair, replay = eng.advance, eng.capture_pair, sampler._CapturedPair.replay

        def counted_advance(src, dst, cond_only=False):
            if not self._capturing:
                self.log.append("E" + "fc"[bool(cond_only)])
            return advance(src, dst, cond_only)

        def counted_capture(za, zb, cond_only=False):
            self.log.append("C" + "fc"[bool(cond_only)])
            self._capturing = True
            try:
                pair = capture_pair(za, zb, cond_only)
            finally:
                self._capturing = False
            self._kind[id(pair)] = (pair, "fc"[bool(cond_only)])     # the pair is kept: its id stays its own
            return pair

        def counted_replay(pair):
            self.log.append("R" + self._kind[id(pair)][1])
            return replay(pair)

        monkeypatch.setattr(eng, "advance", counted_advance)
        monkeypatch.setattr(eng, "capture_pair", counted_capture)
        monkeypatch.setattr(sampler._CapturedPair, "replay", counted_replay)

    def take(self):
        out, self.log = self.log, []
        return out


def _chain(eng, z, sched, dev):
    """the trajectory by hand: ``step`` with explicit timesteps; dpmpp_2m gets t_last = None first, then the previous t_now"""
    B, x = z.shape[0], z.clone()
    for i in range(sched.numel() - 1):
        tl = None if eng.solver == "ddim" or i == 0 else ts([int(sched[i - 1])] * B, dev)
        x = eng.step(x, ts([int(sched[i])] * B, dev), ts([int(sched[i + 1])] * B, dev), t_last=tl)
    return x


@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
@pytest.mark.parametrize("target", ["video", "audio"])
def test_short_trajectories(dev, model, monkeypatch, target, solver):
    z, zp, npr = video_case(dev, B=2, W=32) if target == "video" else audio_case(dev, B=2, L=40)
    eng = engine(model[1], target, tuple(z.shape), npr, guidance=G, solver=solver)
    eng.set_prompt(zp)
    assert 2 * z.shape[0] * eng.N == (296 if target == "video" else 72) < eng.GRAPH_BELOW_ROWS     # graph=None replays here
    ev = Events(eng, monkeypatch)
    for n_steps in (1, 2, 3, 4, 5):
        sched = R.sampling_schedule(1000, n_steps)
        ref = _chain(eng, z, sched, dev)
        assert ev.take() == []                                     # step() is none of the three
        for graph, want in ((False, EAGER), (True, GRAPH), (None, GRAPH)):
            out = eng.run(z, sched, graph=graph)
            got = ev.take()
            print(f"{target} {solver} n_steps={n_steps} graph={graph}: {''.join(e[0] for e in got)}")
            assert torch.equal(out, ref), (n_steps, graph)
            assert "".join(e[0] for e in got) == want[n_steps] and all(e[1] == "f" for e in got), (n_steps, graph, got)
    # a schedule of one entry has no steps: a copy of z, nothing launched
    for graph in (False, True):
        out = eng.run(z, torch.tensor([-1]), graph=graph)
        assert torch.equal(out, z) and out.data_ptr() != z.data_ptr() and ev.take() == []


def test_guidance_interval_events(dev, model, monkeypatch):
    z, zp, npr = video_case(dev, B=2, W=32)
    sched = R.sampling_schedule(1000, 8)
    assert sched.tolist() == [999, 874, 749, 624, 499, 374, 249, 124, -1]
    eng = engine(model[1], "video", tuple(z.shape), npr, guidance=G, guidance_interval=(300, 800))
    eng.set_prompt(zp)
    ev = Events(eng, monkeypatch)
    zg = eng.run(z, sched, graph=True)
    got = ev.take()
    print("interval (300, 800), graph=True:", " ".join(got))
    # cond [0, 2), cfg [2, 6), cond [6, 8): each kind warms up on its own and keeps its own pair
    assert got == "Ec Ec Ef Cf Rf Ef Cc Rc".split()
    ze = eng.run(z, sched, graph=False)
    assert ev.take() == "Ec Ec Ef Ef Ef Ef Ec Ec".split()
    assert torch.equal(zg, ze)
