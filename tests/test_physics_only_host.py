"""Physics-only mode (HS_FLAG_EXT_SKIP_OBSERVATIONS, the oracle's skip_observations) on the CPU oracle alone: the
fixtures of tests/test_gpu_physics_only.py are not vacuous, the mode is not the default step, and the oracle's rewards
follow a float64 rule that is derived from neither the oracle nor a kernel.

Without the observation pass nothing lowers hiderTeamReward between two steps (sim.cpp:700-705 does not run), so the
flag that outputRewardsDonesSystem reads is what rewardsVisSystem alone made of the poses after physics
(sim.cpp:763-841): from episode step 95 on every world casts its seeker -> hider rays inside the physics step, on every
step.  The helpers here take a *side* (lockstep: a RefSim or a GpuSide), so the GPU file runs the same code on the
device.

The figures in the docstrings were measured on the oracle; the floors are about three quarters of them."""
import numpy as np
import pytest

import lockstep
import observe_f64 as O
from lockstep import EXT_SKIP_OBSERVATIONS
from test_observations_float64 import CAP, EPS_COS, EPS_EULER, EPS_T

SEEKER, HIDER = 0, 1                  # self_type

# name -> (constructor arguments, action stream, stream seed, steps, floors)
SCENARIOS = {
    "A": (dict(worlds=16, seed=0), "bench", 1234, 250, dict(seen=1000, unseen=750, regenerated=16, first=4, second=4)),
    "B": (dict(worlds=8, flags=13, seed=5, hiders=(3, 3), seekers=(3, 3)), "full", 1234, 250,
          dict(seen=400, unseen=450, penalty=100, first=2, second=2)),
    "C": (dict(worlds=24, seed=8, hiders=(1, 3), seekers=(1, 3)), "full", 1234, 250,
          dict(seen=1100, unseen=1500, regenerated=24)),
    "D": (dict(worlds=19, seed=0), "full", 7, 140, dict(seen=250, unseen=190, regenerated=70)),
}
D_SAVE, D_LOAD = 120, 128             # scenario D: before these loop steps, save every world / load the even worlds

# the float64 rule: 16 worlds, stream("full", 99), dumps after these loop steps (episode steps 95, 101, .., 233, 238)
RULE_SCENES = {"2+2": (dict(worlds=16, flags=0, seed=3), dict(seen=150, unseen=120)),
               "3+3": (dict(worlds=16, flags=13, seed=5, hiders=(3, 3), seekers=(3, 3)), dict(seen=150, unseen=120, penalty=90))}
RULE_STREAM = ("full", 99)
RULE_DUMPS = tuple(range(95, 234, 6)) + (238,)


def seen_unseen(reward, self_type, self_mask, worlds):
    """Per world, from a side's exports: (a hider row has reward -1 or -11, a hider row has reward +1 or -9).  Under the
    flag the visible_* exports stay zero, so the reward is the only export that says what the rays decided."""
    r = np.asarray(reward).reshape(worlds, -1)
    hider = (np.asarray(self_type).reshape(worlds, -1) == HIDER) & (np.asarray(self_mask).reshape(worlds, -1) != 0)
    return (hider & ((r == -1) | (r == -11))).any(1), (hider & ((r == 1) | (r == -9))).any(1)


def d_resets(s, worlds):
    """Scenario D: from step 100 on, on every third step, a reset is requested for the worlds with (w + s) % 3 == 0."""
    if s >= 100 and s % 3 == 0:
        return ((np.arange(worlds) + s) % 3 == 0).astype(np.int32)
    return np.zeros(worlds, np.int32)


class Tally:
    """World-steps by what the exports of a side say, summed over the steps of a run."""

    def __init__(self, side, worlds):
        self.side, self.n = side, worlds
        self.c = dict(seen=0, unseen=0, penalty=0, regenerated=0, first=0, second=0, draws=0)
        self.keys = set()
        self.resync()

    def _key(self):
        return self.side.tensor("seed").reshape(self.n, -1, 2)[:, 0, 0].copy()

    def resync(self):
        """The teams and episode keys as they are now (at the start, and after a checkpoint load)."""
        self.key = self._key()
        self.keys.update(self.key.tolist())
        self.kind, self.mask = self.side.tensor("self_type").copy(), self.side.tensor("self_mask").copy()

    def step(self):
        """After a step of the side.  The rewards belong to the teams the step worked on, those before it."""
        reward = self.side.tensor("reward")
        seen, unseen = seen_unseen(reward, self.kind, self.mask, self.n)
        r = reward.reshape(-1)
        c = self.c
        c["seen"] += int(seen.sum())
        c["unseen"] += int(unseen.sum())
        c["penalty"] += int(((self.mask.reshape(-1) != 0) & ((r == -11) | (r == -9))).sum())
        done = self.side.tensor("done").reshape(self.n, -1)[:, 0] == 1
        res = self.side.tensor("episode_result")[done]
        c["first"] += int((res[:, 0] == 1).sum())
        c["second"] += int((res[:, 1] == 1).sum())
        c["draws"] += int((res[:, 0] == 0.5).sum())
        key = self._key()
        c["regenerated"] += int((key != self.key).sum())
        self.resync()
        return seen, unseen

    def floors(self, want, tag):
        print(f"{tag}: {self.c}, episode keys {sorted(self.keys)}")
        for k, v in want.items():
            assert self.c[k] >= v, (tag, k, self.c[k], v)


def reward_rule(side, worlds, A, tag=""):
    """The float64 rule on one dump of a side stepped under the flag: for every world whose last step worked on
    episode step >= 95 and did not regenerate it, the hiders' reward is -1 iff a seeker -> hider bit of the restatement
    of the dumped state (no `prev`: the flag has no history) is set, the seekers get the negative, and -10 applies
    where the restatement says the agent is beyond |x|, |y| = 18.  Rows are compared, exactly, where one robust bit
    says seen or every bit robustly says unseen, and the bound is farther than EPS_T * 18.  Returns the counts:
    live / seen / unseen / left (out) world-steps, penalty and compared rows."""
    b, m = side.bodies()
    w, info = side.walls()
    team, mask, reward = side.tensor("self_type"), side.tensor("self_mask"), side.tensor("reward")
    res = O.observe(b, m, w, info, team, A)
    live = np.asarray(info)[:, 6] >= O.PREP_STEPS              # the step before worked on this minus one, no regeneration
    rows = np.repeat(live, A)
    assert np.array_equal(res["active"][rows], mask.reshape(-1)[rows] != 0), (tag, "self_mask")
    pairs, vis = O.seen(res, team, A), res["visible_agents_mask"][:, :, 0] == 1
    good = O.robust(res, EPS_COS, EPS_T, EPS_EULER)["visible_agents_mask"]
    seen = (pairs & vis).reshape(worlds, -1).any(1)
    decided = (pairs & vis & good).reshape(worlds, -1).any(1) | (~pairs | (~vis & good)).reshape(worlds, -1).all(1)
    flag = np.repeat(np.where(seen, -1.0, 1.0), A)
    want = np.where(team.reshape(-1) == SEEKER, -flag, flag) - 10.0 * res["reward_penalty"]
    act = rows & res["active"]
    keep = act & np.repeat(decided, A) & (res["margin"]["reward_bound"] > EPS_T * 18)
    got = np.asarray(reward, np.float64).reshape(-1)
    bad = np.flatnonzero(keep & (got != want))
    assert not len(bad), (tag, "rows", bad[:8].tolist(), "reward", got[bad[:8]].tolist(), "float64 rule", want[bad[:8]].tolist())
    left = live & (act & ~keep).reshape(worlds, A).any(1)
    return dict(live=int(live.sum()), seen=int((live & seen).sum()), unseen=int((live & ~seen).sum()), left=int(left.sum()),
                penalty=int((act & res["reward_penalty"]).sum()), rows=int(keep.sum()))


def rule_scene(side, step, act, worlds, A, tag, dumps=RULE_DUMPS):
    """Drive a side with RULE_STREAM and apply reward_rule after each loop step of `dumps`; the summed counts."""
    draw, _ = lockstep.stream(*RULE_STREAM)
    total = {}
    for s in range(max(dumps) + 1):
        act(draw(s, worlds * A))
        step()
        if s in dumps:
            for k, v in reward_rule(side, worlds, A, f"{tag}, after step {s}").items():
                total[k] = total.get(k, 0) + v
    return total


def rule_floors(total, want, tag, dumps=RULE_DUMPS):
    print(f"{tag}: {total}; left out {total['left']} of {total['live']} live world-steps "
          f"({100.0 * total['left'] / max(1, total['live']):.2f} %)")
    assert total["live"] == 16 * len(dumps), (tag, total)
    assert total["left"] <= CAP * total["live"], (tag, total)
    for k, v in want.items():
        assert total[k] >= v, (tag, k, total[k], v)


def _ref(kw, flags=EXT_SKIP_OBSERVATIONS):
    kw = dict(kw)
    ref = lockstep.make_ref(kw.pop("worlds"), flags=kw.pop("flags", 0) | flags, threads=4, **kw)
    ref.init()
    return ref


def _checkpoints(ref, trigger, load):
    ref.tensor("ckpt_ctrl")[:, 0] = trigger
    ref.load_checkpoints() if load else ref.save_checkpoints()
    ref.tensor("ckpt_ctrl")[:] = 0


def _run(name, flags=EXT_SKIP_OBSERVATIONS):
    """Scenario `name` on the oracle: the tally, and the rewards and episode results after every step."""
    kw, kind, stream_seed, steps, _ = SCENARIOS[name]
    ref = _ref(kw, flags)
    n = kw["worlds"]
    draw, cols = lockstep.stream(kind, stream_seed)
    tally = Tally(ref, n)
    rewards, results = [], []
    for s in range(steps):
        if name == "D":
            if s == D_SAVE:
                _checkpoints(ref, 1, load=False)
            if s == D_LOAD:
                _checkpoints(ref, (np.arange(n) % 2 == 0).astype(np.int32), load=True)
                tally.resync()
            ref.tensor("reset")[:, 0] = d_resets(s, n)
        a = draw(s, n * ref.A)
        if cols is None:
            ref.tensor("action")[:] = a
        else:
            ref.tensor("action")[:, list(cols)] = a
        ref.step()
        tally.step()
        rewards.append(ref.tensor("reward").copy())
        results.append(ref.tensor("episode_result").copy())
    if flags & EXT_SKIP_OBSERVATIONS:       # self_type and self_mask are the level generator's, not the observation pass's
        for obs in set(lockstep.OBS) - {"self_type", "self_mask"}:
            assert not ref.tensor(obs).any(), (obs, "is written although observations are skipped")
    ref.close()
    return tally, rewards, results


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_scenarios_reach_both_outcomes(oracle, name):
    """Measured, the episode's last step included: A seen 1 304, unseen 1 016 world-steps, 16 regenerations, results
    8 / 8 / 0 draws; B 520 / 640, 134 rows with the -10 penalty, results 3 / 5; C 1 462 / 2 018, 24 regenerations;
    D 342 / 254, 91 regenerations."""
    tally, _, _ = _run(name)
    tally.floors(SCENARIOS[name][4], f"scenario {name}, physics-only, oracle")


def test_the_mode_is_not_the_default_step(oracle):
    """Scenario B with and without the flag: the reference's visibility pass lowers the team flag as a side effect, so
    rewards (measured: in 65 steps) and even episode results (in the one step that shows them) differ.  The GPU test therefore pins the
    mode, not the default step."""
    _, r1, e1 = _run("B")
    _, r0, e0 = _run("B", flags=0)
    rewards = sum(not np.array_equal(lockstep.bits(a), lockstep.bits(b)) for a, b in zip(r0, r1))
    results = sum(not np.array_equal(lockstep.bits(a), lockstep.bits(b)) for a, b in zip(e0, e1))
    print(f"scenario B, default against physics-only: rewards differ in {rewards} steps, episode_result in {results}")
    assert rewards >= 30 and results >= 1, (rewards, results)


@pytest.mark.parametrize("scene", list(RULE_SCENES))
def test_float64_rule_on_the_oracle(oracle, scene):
    """Measured: 400 live world-steps per scene and none left out; 2+2 has 225 seen and 175 unseen, 3+3 has 152 seen,
    248 unseen and 127 penalty rows; no mismatch."""
    kw, want = RULE_SCENES[scene]
    ref = _ref(kw)

    def act(a):
        ref.tensor("action")[:] = a
    total = rule_scene(ref, ref.step, act, kw["worlds"], ref.A, f"rule scene {scene}, oracle")
    ref.close()
    rule_floors(total, want, f"rule scene {scene}, oracle")
