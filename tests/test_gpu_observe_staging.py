"""k_observe's staging copy, agent table and cull on the device, lock-step against the CPU oracle: every exported
observation tensor (and the rest of lockstep.NAMES, bodies and walls) bit for bit after every step.

stage_world moves a world's columns into LDS with one table-driven copy whose source offsets depend on the octet, the
slot inside it and the block -> world mapping of the grid; the agent table has an item per (agent, other body); the cull
reads a threshold per (agent, body).  The shapes are the smallest that reach every path of that code:
  * 1, 9 and 65 worlds: a lone world beside seven empty slots, a partial second octet, and the first world of the
    second group of 8 octets (block 64);
  * 1+1, 2+2, 3+2 and 3+3 agents: k_observe<128>, <192> and <320>, a table that ends inside a wave and one that fills
    waves exactly, all 6 agent slots;
  * a balance deal (slots != world ids afterwards), a world with many walls, debug levels with three planes, and a reset
    of one world between two others that go on.
"""
import numpy as np
import pytest

import scenes
from lockstep import Pair

pytestmark = pytest.mark.gpu

TEAMS = [((1, 1), (1, 1)), ((2, 2), (2, 2)), ((3, 3), (2, 2)), ((3, 3), (3, 3))]


@pytest.mark.parametrize("worlds", [1, 9, 65])
@pytest.mark.parametrize("hiders,seekers", TEAMS, ids=["1+1", "2+2", "3+2", "3+3"])
def test_worlds_and_team_sizes(oracle, worlds, hiders, seekers):
    """12 steps from init with random move / grab / lock actions; checked at init and after every step."""
    p = Pair(worlds, seed=31, hiders=hiders, seekers=seekers)
    assert p.sim.agents_per_world == hiders[1] + seekers[1]
    p.check("init")
    p.drive(12, "full", seed=worlds)
    assert np.isfinite(p.ref.tensor("self_data")).all()


def test_across_a_balance_deal(oracle):
    """24 worlds, 2+2, 40 steps: the deal after step 32 moves the worlds to other slots, so the slot headers, not the
    world ids, say what a workgroup stages."""
    p = Pair(24, seed=32)
    p.drive(40, "full", seed=5)


def test_across_a_deal_with_a_partial_last_octet(oracle):
    """19 worlds, 2+2, 70 steps: two full octets, which the deals after steps 32 and 64 shuffle, and three worlds in a
    partial last octet, which must stay in their slots (k_balance_move_all and k_balance_commit with nfull < N)."""
    p = Pair(19, seed=32)
    p.drive(70, "full", seed=5)


def test_world_with_the_most_walls(oracle):
    """Among 32 generated levels the one with the most walls, its first agent moved to the spot farthest from every
    wall (scenes.open_spot) so that its lidar rays reach walls on all sides; the same in every other world.  4 steps."""
    p = Pair(32, seed=33)
    walls, info = p.sim.debug_walls()
    count = info[:, 0].astype(int)
    most = int(count.argmax())
    assert count[most] >= 24 and count.min() >= 1, count       # (28 of at most 36 in world 30)

    def edit(rec, meta):
        for w in range(len(rec)):
            x, y, clear = scenes.open_spot(walls[w], count[w])
            a = rec[w]["agents"][0]
            scenes.put(a, (x, y, float(a["pos"][2])), rot=scenes.yaw_quat(0.3 + w))
    scenes.inject(p, edit)
    lidar = p.ref.tensor("lidar").reshape(32, 4, 30)[most, 0]
    assert (lidar > 0).all(), "every lidar ray of the moved agent ends on something"
    p.drive(4, "full", seed=6)


@pytest.mark.parametrize("level", [6, 7])
def test_debug_levels_with_a_wall_and_with_three_planes(oracle, level):
    """Debug level 7 has three planes (the floor and two side planes) and level 6 two agents, a cube and a long wall:
    every staged plane row and the counts of the slot header, 4 steps each."""
    p = Pair(3, flags=2, level=level, hiders=(1, 1), seekers=(1, 1))
    assert (p.sim.debug_walls()[1][:, 1] == (3 if level == 7 else 1)).all(), "plane count"
    p.check("init")
    p.drive(4, "none")


def test_one_world_resets_between_others(oracle):
    """9 worlds; world 4 is reset by the host before step 3: the launch that observes it stages the header and the
    geometry of a level generated in the same step, the other worlds carry on."""
    p = Pair(9, seed=34)
    rng = np.random.default_rng(7)
    for s in range(6):
        if s == 3:
            p.ref.tensor("reset")[4] = 1
            p.gpu.view("reset")[4] = 1
        a = np.stack([rng.integers(0, 11, p.rows), rng.integers(0, 11, p.rows), rng.integers(0, 11, p.rows),
                      rng.integers(0, 2, p.rows), rng.integers(0, 2, p.rows)], axis=1)
        p.step(a)
        p.check(f"step {s}")
    seed = p.ref.tensor("seed").reshape(9, 4, 2)
    assert (seed[4, :, 0] == 1).all() and (np.delete(seed, 4, axis=0)[:, :, 0] == 0).all(), "only world 4 began a second episode"
