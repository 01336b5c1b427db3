"""The reward's line of sight (rewardsVisSystem, src/sim.cpp:763-804) is taken from k_observe's agent-visibility rays
wherever a k_observe follows the physics step on the same state (csrc/hs_k_physics.h phase_post, csrc/hs_k_observe.h):
k_physics writes rewards and running scores as for "no hider seen" and marks the slot header, k_observe rewrites them
when one of its seeker -> hider rays hits.  Everything the reference derives from that flag — reward, done,
episode_result, and the running scores a checkpoint carries — must stay bit-equal to the CPU oracle after every step."""
import numpy as np
import pytest

from lockstep import Pair, bits

pytestmark = pytest.mark.gpu

PREP_LAST = 95                        # the first episode step whose reward reads the flag
SEEKER, HIDER = 0, 1                  # self_type
IGNORE_EPISODE_LENGTH = 2             # SimFlags
SCORES = slice(2, 4)                  # hs_checkpoint::running_scores, in int32 words of a record
STEP_WORD = 4                         # hs_checkpoint::episode_step


def _bench_stream(rows):
    """bench.py's actions: zero moves for the first step, then default_rng(0).integers(-5, 5) into columns 0-1."""
    rng = np.random.default_rng(0)
    yield np.zeros((rows, 2), np.int64)
    while True:
        yield rng.integers(-5, 5, size=(rows, 2))


def _seen(ref, worlds):
    """Per world: a seeker -> hider entry of the oracle's visible_agents_mask is set."""
    A = ref.A
    vis = ref.tensor("visible_agents_mask").reshape(worlds, A, 5) != 0
    kind = ref.tensor("self_type").reshape(worlds, A)
    live = ref.tensor("self_mask").reshape(worlds, A) != 0
    out = np.zeros(worlds, bool)
    for i in range(A):
        for jj in range(A - 1):
            j = jj if jj < i else jj + 1
            out |= vis[:, i, jj] & live[:, i] & live[:, j] & (kind[:, i] == SEEKER) & (kind[:, j] == HIDER)
    return out


class _Run:
    """A Pair stepped under one action stream; after every step the tensors the flag feeds are compared."""

    def __init__(self, worlds, stream=_bench_stream, **kw):
        import torch
        self.torch = torch
        self.p = Pair(worlds, **kw)
        self.n = worlds
        self.acts = stream(self.p.rows)
        self.ctrl = self.p.sim.ckpt_ctrl_tensor().to_torch().view(torch.int32)
        self.ck = self.p.sim.ckpt_tensor().to_torch()
        self.steps = 0
        self.seen = _seen(self.p.ref, worlds)             # after the previous step (here: after init)
        self.counts = dict(first=0, already=0, neither=0, regenerated=0)
        self.first_sight = np.zeros(worlds, bool)         # of the last step

    def scores(self):
        """(GPU, oracle) running scores, through a save of every world's checkpoint."""
        self.ctrl[:] = 1
        self.p.ref.tensor("ckpt_ctrl")[:] = 1
        self.p.sim.save_checkpoints(); self.p.ref.save_checkpoints()
        g = self.ck.cpu().numpy().view(np.int32).reshape(self.n, 348)[:, SCORES].copy()
        r = self.p.ref.tensor("ckpt").view(np.int32).reshape(self.n, 348)[:, SCORES].copy()
        return g, r

    def compare(self, tag, names=("reward", "done", "episode_result")):
        self.p.check(tag, names=names, bodies=False, walls=False)
        g, r = self.scores()
        assert np.array_equal(g, r), (tag, "running_scores", np.argwhere(g != r)[:4].tolist())

    def step(self, names=("reward", "done", "episode_result"), resets=None):
        p = self.p
        if resets is not None:
            p.ref.tensor("reset")[:, 0] = resets
            p.gpu.view("reset")[:, 0] = self.torch.from_numpy(resets.astype(np.int32)).to(p.gpu.view("reset").device)
        info = p.ref.walls()[1]
        ep = info[:, 6].copy()                               # the episode step this step works on, per world
        p.step(next(self.acts), (0, 1))
        now = _seen(p.ref, self.n)
        regen = p.ref.walls()[1][:, 6] == 0
        live = (ep >= PREP_LAST) & ~regen
        self.first_sight = live & now & ~self.seen
        self.counts["first"] += int(self.first_sight.sum())
        self.counts["already"] += int((live & self.seen).sum())
        self.counts["neither"] += int((live & ~now & ~self.seen).sum())
        self.counts["regenerated"] += int(regen.sum())
        self.seen = now
        self.compare(f"step {self.steps}", names)
        self.steps += 1


def test_bench_recipe_over_an_episode_matches_the_oracle(oracle):
    """16 worlds, 2 + 2, seed 0, 250 steps of the benchmark's actions: past the end of the preparation phase and the
    regeneration of every level.  The oracle alone gives 5 first-sight, 1 136 already-seen and 1 163 unseen world-steps
    with episode step in [95, 238], and 16 regenerations."""
    r = _Run(16, seed=0)
    for _ in range(250):
        r.step()
    c = r.counts
    print(c)
    assert c["first"] >= 3 and c["already"] >= 100 and c["neither"] >= 100 and c["regenerated"] >= 16, c


def test_three_hiders_and_three_seekers(oracle):
    """k_physics<3> and k_observe<320>: 8 worlds, 130 steps."""
    r = _Run(8, seed=0, hiders=(3, 3), seekers=(3, 3))
    for _ in range(130):
        r.step()
    c = r.counts
    print(c)
    assert c["first"] >= THREE_PLUS_THREE["first"] and c["already"] >= THREE_PLUS_THREE["already"] and \
        c["neither"] >= THREE_PLUS_THREE["neither"], c


# the oracle alone gives {first: 4, already: 177, neither: 99} for the run above; the test asks for the better part of it
THREE_PLUS_THREE = dict(first=3, already=100, neither=50)


def test_the_mark_is_consumed_once(oracle):
    """Right after a step with a first sight: observations are recomputed without a physics step in front (a checkpoint
    load of the OTHER worlds, then of every world).  Rewards, episode results and running scores stay what they were,
    and the run stays in lock-step."""
    import torch
    r = _Run(16, seed=0)
    while not r.first_sight.any():
        r.step()
        assert r.steps < 250, "no first sight in the fixture"
    assert r.steps > PREP_LAST
    p = r.p
    reward = p.gpu.tensor("reward").copy()
    result = p.gpu.tensor("episode_result").copy()
    scores, _ = r.scores()                                   # (the save also leaves the records to load from)
    for trig in ((~r.first_sight).astype(np.int32), np.ones(16, np.int32)):
        assert trig.any()
        r.ctrl[:, 0] = torch.from_numpy(trig).to(r.ctrl.device)
        p.ref.tensor("ckpt_ctrl")[:, 0] = trig
        p.sim.load_checkpoints(); p.ref.load_checkpoints()
        r.ctrl[:] = 0; p.ref.tensor("ckpt_ctrl")[:] = 0
        assert np.array_equal(bits(p.gpu.tensor("reward")), bits(reward))
        assert np.array_equal(bits(p.gpu.tensor("episode_result")), bits(result))
        again, ref_scores = r.scores()
        assert np.array_equal(again, scores) and np.array_equal(ref_scores, scores)
        p.check("after the load")
    for _ in range(12):
        r.step()
    p.check("12 steps on")


def test_requested_resets_inside_an_octet(oracle):
    """Worlds whose reset is requested cast their own rays while their neighbours in the octet defer: resets of a
    changing third of the worlds on every third step from step 100 on (the oracle alone: 60 regenerations, 146 unseen and
    243 already-seen world-steps, 3 first sights)."""
    r = _Run(16, seed=0)
    none = np.zeros(16, np.int64)
    for s in range(130):
        want = s >= 100 and s % 3 == 0
        r.step(resets=((np.arange(16) + s) % 3 == 0).astype(np.int64) if want else none)
    assert r.counts["regenerated"] >= 40 and r.counts["neither"] >= 100, r.counts
    r.p.check("end")


def test_ignored_episode_length_past_step_240(oracle):
    """Under IgnoreEpisodeLength no step regenerates the level: steps 236 .. 247 (the counter planted through a
    checkpoint) all defer."""
    n = 16
    r = _Run(n, seed=0, flags=IGNORE_EPISODE_LENGTH)
    for _ in range(3):
        r.step()
    r.scores()
    r.ck.view(r.torch.int32).view(n, 348)[:, STEP_WORD] = 236
    r.p.ref.tensor("ckpt").view(np.int32).reshape(n, 348)[:, STEP_WORD] = 236
    r.ctrl[:] = 1; r.p.ref.tensor("ckpt_ctrl")[:] = 1
    r.p.sim.load_checkpoints(); r.p.ref.load_checkpoints()
    r.ctrl[:] = 0; r.p.ref.tensor("ckpt_ctrl")[:] = 0
    r.p.check("planted")
    for _ in range(12):
        r.step()
    assert (r.p.ref.walls()[1][:, 6] == 248).all() and r.counts["regenerated"] == 0
    assert r.counts["already"] + r.counts["neither"] + r.counts["first"] == 12 * n
    r.p.check("end")
