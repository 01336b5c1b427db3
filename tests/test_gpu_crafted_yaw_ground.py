"""Agents' floor contacts on the device.  An agent is a yaw-only body: its ground manifold gets a manifold-level normal
part (yaw_ground_prepass, hs_solver.h) and then one static-friction correction per point, and that correction yaws the
agent, so a point's lever arm has to be taken after the corrections of the points before it while the point's position at
the substep's start does not change.  Here every agent of every world is written through the Checkpoint record
(oracle/scenes.py) onto the floor next to the world's wall-free spot: pressed up to 8 cm into it, with a random yaw and
a horizontal velocity of up to 3 m/s, so that the static-friction branch is taken for some points and not for others;
every eighth agent hovers 1 cm above the floor (no touching point), and in every fourth world agent 0 stands against a
wall as well, so that its wall manifold is solved behind its ground manifold.  Two steps, every exported tensor, bodies
and walls bit for bit against the oracle; with 2 + 2 agents (k_physics<2>) and with 3 + 3 (k_physics<3>).  With all of
an octet's agents crafted, each of its rounds of bodies holds some."""
import functools
import math

import numpy as np
import pytest

import lockstep
import scenes
import test_gpu_crafted_clipping as clip

WORLDS, SEED, STEPS = 64, 2, 2
DT = 1.0 / 30.0
TEAMS = {"2+2": ((2, 2), (2, 2)), "3+3": ((3, 3), (3, 3))}
# agents around the spot: a 3 x 2 grid, 3.2 m apart (an agent's hull is a 2 m cube: no two of them touch)
GRID = [(-3.2, -1.6), (0.0, -1.6), (3.2, -1.6), (-3.2, 1.6), (0.0, 1.6), (3.2, 1.6)]


def make_ref(teams):
    ref = lockstep.make_ref(WORLDS, flags=0, seed=SEED, hiders=TEAMS[teams][0], seekers=TEAMS[teams][1])
    ref.init()
    return ref


@functools.lru_cache(maxsize=None)
def plan(teams):
    """[(world, agent, pos, yaw, lin, kind)] with kind in "pressed", "hover", "wall"; float64, seeded."""
    ref = make_ref(teams)
    walls, info = ref.walls()
    agents = ref.A
    ref.close()
    rng = np.random.default_rng(77)
    out = []
    for w in range(WORLDS):
        x, y, _ = scenes.open_spot(walls[w], info[w, 0])
        spots = clip.wall_spots(walls[w], int(info[w, 0]), scenes.CUBE, None) if w % 4 == 0 else []
        for a in range(agents):
            yaw = rng.uniform(-math.pi, math.pi)
            speed, heading = rng.uniform(0.0, 3.0), rng.uniform(-math.pi, math.pi)
            lin = np.array([speed * math.cos(heading), speed * math.sin(heading), 0.0])
            depth = rng.uniform(0.0, 0.08)
            kind = "pressed"
            pos = np.array([x + GRID[a][0], y + GRID[a][1], 1.0 - depth])
            if (w * agents + a) % 8 == 7:
                kind, pos[2] = "hover", 1.01
            elif a == 0 and spots:
                kind = "wall"
                row, side, t = spots[-1]
                yaw = rng.choice([0.0, rng.uniform(-0.3, 0.3)])
                cx, cy, hx, hy = (float(v) for v in row)
                ax = 0 if hx < hy else 1
                pos = np.array([cx, cy, 1.0 - depth])
                pos[ax] += side * (min(hx, hy) + abs(math.cos(yaw)) + abs(math.sin(yaw)) - 0.05)
                pos[1 - ax] += t
            out.append((w, a, pos, yaw, lin, kind))
    return out


def editor(teams):
    def edit(rec, meta):
        for w, a, pos, yaw, lin, _ in plan(teams):
            scenes.put(rec[w]["agents"][a], np.float32(pos), np.float32(scenes.yaw_quat(yaw)), np.float32(lin), np.zeros(3, np.float32))
    return edit


FREE_FALL = -10 * 9.8 / 120.0 ** 2        # what four substeps of gravity alone add to a resting body's height in one step


@functools.lru_cache(maxsize=None)
def oracle_outcome(teams):
    """Oracle alone, one step: per planned agent the ratio of its horizontal displacement to |lin| * DT (0: held by static
    friction; 1: slid freely; NaN for agents slower than 0.5 m/s), and the change of its height."""
    ref = make_ref(teams)
    scenes.inject_ref(ref, editor(teams))
    before = ref.bodies()[0].copy()
    ref.step()
    after = ref.bodies()[0]
    ref.close()
    ratio, dz = [], []
    for w, a, pos, yaw, lin, kind in plan(teams):
        s = scenes.AGENT_SLOT0 + a
        move = np.linalg.norm((after[w, s, :2] - before[w, s, :2]).astype(np.float64))
        speed = np.linalg.norm(lin[:2])
        ratio.append(move / (speed * DT) if speed > 0.5 else np.nan)
        dz.append(float(after[w, s, 2]) - float(before[w, s, 2]))
    return np.array(ratio), np.array(dz)


def check_plan_on_the_cpu(teams):
    """Among the pressed agents static friction holds at least 20 (they move less than a quarter of |lin| * DT) and lets
    at least 20 slide (more than three quarters); all of them are lifted; at least 16 hovering agents fall freely (the
    others of them meet a box of the level); at least 8 agents stand against a wall."""
    kinds = np.array([k for *_, k in plan(teams)])
    ratio, dz = oracle_outcome(teams)
    pressed = kinds == "pressed"
    held, slid = int((ratio[pressed] < 0.25).sum()), int((ratio[pressed] > 0.75).sum())
    free = int((np.abs(dz[kinds == "hover"] - FREE_FALL) < 1e-4).sum())
    print(f"{teams}: pressed {int(pressed.sum())}, held {held}, slid {slid}, hovering in free fall {free}, wall {int((kinds == 'wall').sum())}")
    assert held >= 20 and slid >= 20, (held, slid)
    assert free >= 16, free
    assert (kinds == "wall").sum() >= 8
    assert (dz[pressed] > 0).all(), "the pressed agents are lifted by the floor"


@pytest.mark.parametrize("teams", list(TEAMS))
def test_the_plan_is_not_vacuous_on_the_oracle(oracle, teams):
    """No GPU: check_plan_on_the_cpu."""
    check_plan_on_the_cpu(teams)


@pytest.mark.gpu
@pytest.mark.parametrize("teams", list(TEAMS))
def test_agents_on_the_floor_match_the_oracle(oracle, teams):
    """64 worlds with every agent crafted, two steps, bit for bit after the load and after each step."""
    check_plan_on_the_cpu(teams)
    p = lockstep.Pair(WORLDS, flags=0, seed=SEED, hiders=TEAMS[teams][0], seekers=TEAMS[teams][1])
    scenes.inject(p, editor(teams))
    for s in range(1, STEPS + 1):
        p.step()
        p.check(f"step {s}")
    st = p.sim.device_status()
    p.sim.close(); p.ref.close()
    assert st["dropped_candidate_pairs"] == 0, st
