"""Physics-only mode (HS_FLAG_EXT_SKIP_OBSERVATIONS) and the benchmark's horizon on the device, in lock-step with the
CPU oracle.

Under the flag no k_observe follows k_physics, the reset puts hiderTeamReward back to 1 on every step and nothing
lowers it in between, so phase_post (csrc/hs_k_physics.h) never defers: from episode step 95 on EVERY world casts its
seeker -> hider rays inside k_physics on EVERY step — trace_ray over ResGeom, the nine (seeker, hider) pairs over eight
lanes, R.seen — a path the default mode reaches for a handful of world-steps.  Rewards, dones, episode results and the
running scores a checkpoint carries must equal "the reference's step with the observation nodes removed"
(src/sim.cpp:763-841, 1232-1293), which is what the oracle's skip_observations is; the observation tensors stay zero on
both sides and are compared like every other name of lockstep.NAMES.  The float64 rule of
tests/test_physics_only_host.py, derived from neither side, is then applied to the device alone.

Scenarios, floors and helpers are those of tests/test_physics_only_host.py, which shows on the oracle alone that the
fixtures reach both outcomes and that the mode differs from the default step."""
import numpy as np
import pytest

import lockstep
from lockstep import EXT_SKIP_OBSERVATIONS, Pair
from test_physics_only_host import (D_LOAD, D_SAVE, RULE_DUMPS, RULE_SCENES, SCENARIOS, Tally, d_resets, rule_floors,
                                    rule_scene)

pytestmark = pytest.mark.gpu

SCORES = slice(2, 4)                  # hs_checkpoint::running_scores, in int32 words of a record
RECORD = 348                          # int32 words of a checkpoint record


class _Run:
    """A Pair under one action stream, with the tally taken from the GPU side's exports."""

    def __init__(self, worlds, kind, stream_seed, **kw):
        import torch
        self.torch = torch
        self.p = Pair(worlds, **kw)
        self.n = worlds
        self.draw, self.cols = lockstep.stream(kind, stream_seed)
        self.ctrl = self.p.sim.ckpt_ctrl_tensor().to_torch().view(torch.int32)
        self.ck = self.p.sim.ckpt_tensor().to_torch()
        self.tally = Tally(self.p.gpu, worlds)

    def checkpoints(self, trigger, load=False):
        """Save (or load) the worlds of `trigger` on both sides."""
        p = self.p
        trigger = np.broadcast_to(np.asarray(trigger, np.int32), (self.n,))
        self.ctrl[:, 0] = self.torch.from_numpy(trigger.copy()).to(self.ctrl.device)
        p.ref.tensor("ckpt_ctrl")[:, 0] = trigger
        if load:
            p.sim.load_checkpoints(); p.ref.load_checkpoints()
        else:
            p.sim.save_checkpoints(); p.ref.save_checkpoints()
        self.ctrl[:] = 0; p.ref.tensor("ckpt_ctrl")[:] = 0

    def scores(self, tag):
        """The running scores of both sides, through a save of every world's checkpoint."""
        self.checkpoints(1)
        g = self.ck.cpu().numpy().view(np.int32).reshape(self.n, RECORD)[:, SCORES]
        r = self.p.ref.tensor("ckpt").view(np.int32).reshape(self.n, RECORD)[:, SCORES]
        assert np.array_equal(g, r), (tag, "running_scores", np.argwhere(g != r)[:4].tolist())

    def step(self, s, resets=None):
        p = self.p
        if resets is not None:
            p.ref.tensor("reset")[:, 0] = resets
            dst = p.gpu.view("reset")
            dst[:, 0] = self.torch.from_numpy(resets).to(dst.device)
        p.step(self.draw(s, p.rows), self.cols)
        self.tally.step()


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_scenarios_in_lock_step(oracle, name):
    """A: the benchmark's recipe over an episode and its regeneration.  B: k_physics<3> with all nine pairs, grabs and
    locks (flags 13).  C: team counts below 3, so the `si < cnt_seekers` guards decide which pairs cast, and 24 worlds
    are three octets that k_balance deals at steps 32, 64, ...  Every name of lockstep.NAMES, bodies and walls after
    every step from step 90 on and every 8th before; running scores every 10th step and after the last."""
    kw, kind, stream_seed, steps, floors = SCENARIOS[name]
    kw = dict(kw)
    r = _Run(kw.pop("worlds"), kind, stream_seed, flags=kw.pop("flags", 0) | EXT_SKIP_OBSERVATIONS, **kw)
    for s in range(steps):
        r.step(s)
        if s >= 90 or (s + 1) % 8 == 0:
            r.p.check(f"scenario {name}, step {s}")
        if (s + 1) % 10 == 0 or s == steps - 1:
            r.scores(f"scenario {name}, step {s}")
    r.tally.floors(floors, f"scenario {name}, physics-only, device")


def test_resets_and_checkpoints_with_a_partial_octet(oracle):
    """Scenario D: 19 worlds are two dealt octets plus three worlds that stay in their slots.  From step 100 on a reset
    is requested for a third of the worlds on every third step, inside octets whose other worlds cast their own rays
    too; before step 120 every checkpoint is saved and before step 128 the even worlds are loaded, with no observation
    pass after the load.  Checked after every step; running scores at the save and after the last step."""
    kw, kind, stream_seed, steps, floors = SCENARIOS["D"]
    n = kw["worlds"]
    r = _Run(n, kind, stream_seed, seed=kw["seed"], flags=EXT_SKIP_OBSERVATIONS)
    for s in range(steps):
        if s == D_SAVE:
            r.scores("scenario D, the save")
        if s == D_LOAD:
            r.checkpoints((np.arange(n) % 2 == 0).astype(np.int32), load=True)
            r.p.check("scenario D, after the load")
            r.tally.resync()
        r.step(s, resets=d_resets(s, n))
        r.p.check(f"scenario D, step {s}")
    r.scores("scenario D, the end")
    r.tally.floors(floors, "scenario D, physics-only, device")


@pytest.mark.parametrize("scene", list(RULE_SCENES))
def test_float64_rule_on_the_device(scene):
    """The HIP simulator alone under the flag, its rewards against the float64 restatement of its own dumped state at
    the 25 dumps of the host test.  No tolerance is involved: kept rows are compared exactly, and at most 2 % of the
    live world-steps may be left out as decided too near an edge."""
    import gpu_hideseek
    import torch
    kw, want = RULE_SCENES[scene]
    hiders, seekers = kw.get("hiders", (2, 2)), kw.get("seekers", (2, 2))
    sim = gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=kw["worlds"],
        sim_flags=kw["flags"] | EXT_SKIP_OBSERVATIONS, rand_seed=kw["seed"], min_hiders=hiders[0], max_hiders=hiders[1],
        min_seekers=seekers[0], max_seekers=seekers[1], num_pbt_policies=1)
    sim.init()
    side = lockstep.GpuSide(sim)
    dst = side.view("action")

    def act(a):
        dst.copy_(torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dst.device))
    total = rule_scene(side, sim.step, act, kw["worlds"], sim.agents_per_world, f"rule scene {scene}, device")
    sim.close()
    rule_floors(total, want, f"rule scene {scene}, device")


@pytest.mark.parametrize("flags", [0, EXT_SKIP_OBSERVATIONS], ids=["default", "physics-only"])
def test_the_benchmarks_horizon(oracle, flags):
    """1 920 steps of the benchmark's actions on 24 worlds: 8 episodes, episode keys 0..8 and 60 deals of k_balance.
    Every name, bodies, walls and the running scores after every 64th step, after the last step of every episode, after
    the step that follows it, and after the last step.  The oracle alone gives 192 regenerations, results 109 / 83 / 0
    (default) and 109 / 82 / 1 (physics-only), and 12 046 / 15 794 and 11 917 / 15 923 seen / unseen world-steps."""
    n, steps = 24, 1920
    r = _Run(n, "bench", 1234, seed=0, threads=8, flags=flags)
    for s in range(steps):
        r.step(s)
        if (s + 1) % 64 == 0 or (s + 1) % 240 == 0 or (s and s % 240 == 0) or s == steps - 1:
            r.p.check(f"step {s}")
            r.scores(f"step {s}")
    r.tally.floors(dict(seen=9000, unseen=12000), f"the benchmark's horizon, flags {flags}, device")
    assert r.tally.c["regenerated"] == 192, r.tally.c
    assert r.tally.keys == set(range(9)), sorted(r.tally.keys)
