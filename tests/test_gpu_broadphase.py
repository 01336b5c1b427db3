"""The k_physics broadphase on scenes made for it: walls pre-selected through strip masks, each pair of body slots
tested once (marl-hideandseek_amd/csrc/hs_broadphase.h, phase_detect).  Scenes are written through the Checkpoint
record (oracle/scenes.py) and stepped in lock step with the oracle, bit for bit, every world.  Each GPU test has a twin
without a GPU that asserts on the oracle alone that the scene holds what it claims.

Walls beyond the 32 staged ones: levels with more than 32 walls did not occur among 200 000 generated worlds (seed 0:
5 .. 31 walls, one world with 31), and walls are not part of a Checkpoint record, so no scene here reaches the loop over
wall indices >= 32; tests/test_broadphase_host.py covers it with 33 and 36 walls.  The wall-count scene below takes the
widest range found instead (31 and 8 walls in one octet)."""
import numpy as np
import pytest

import lockstep
import scenes

WORLDS = 9                      # one full octet and an octet with seven empty slots
SEED = 0
STEPS = 8
TEAMS = {"two_slots_per_lane": ((2, 2), (2, 2)), "three_slots_per_lane": ((3, 3), (3, 3))}    # k_physics<2> / k_physics<3>
STRIP = 5.0                     # hs_broadphase.h strip_of: boundaries at -15, -10 .. 15
DD_CAPACITY = 16                # body-body candidates a world keeps in LDS (hs_dev.h kMaxDDCand)
MARGIN = 1e-3                   # float64 AABBs here, float32 on both sides: count only what is clear of rounding
FAR = (40.0, -35.0)             # outside the outer walls (which lie at +-18)
INNER = 17.8                    # inner faces of the outer walls (half thickness 0.2)


def crafted_editor(walls, info, roles):
    """Per world: the first elongated box yawed by 45 degrees into the (-x, -y) corner of the outer walls, its two ends
    0.1 m inside either wall; the last box or ramp far outside the walls; the one before it against the +x outer wall
    (beyond the last strip boundary, 0.1 m inside the wall); every other body in a pile around the strip corner nearest to the world's most
    open spot: the first of them centred exactly on the corner, the agents (the highest slots) inside the pile.
    `roles[w]` receives the slots."""
    def edit(rec, meta):
        rng = np.random.default_rng(5)
        for w in range(len(rec)):
            live = [s for s in range(scenes.AGENT_SLOT0) if meta[w, s, 0] >= 0]
            long_box = next(s for s in live if meta[w, s, 0] == scenes.BOX)
            rest = [s for s in live if s != long_box]
            far, near, pile = rest[-1], rest[-2], rest[:-2]
            q45 = np.float32(scenes.yaw_quat(np.pi / 4))
            reach = scenes.hull_vertices(scenes.BOX, (0, 0, 0), q45)[:, 0].max()
            r = scenes.slot_record(rec[w], long_box)
            c = -(INNER + 0.1) + reach
            scenes.put(r, np.float32([c, c, r["pos"][2]]), q45, locked=False)
            r = scenes.slot_record(rec[w], far)
            scenes.put(r, np.float32([FAR[0], FAR[1], r["pos"][2]]), locked=False)
            r = scenes.slot_record(rec[w], near)
            half = scenes.hull_vertices(int(meta[w, near, 0]), (0, 0, 0), (1, 0, 0, 0))[:, 0].max()
            k = next(k for k in range(info[w, 0]) if walls[w, k, 0] > 17 and walls[w, k, 2] < 0.5)     # a piece of the +x outer wall
            scenes.put(r, np.float32([walls[w, k, 0] - walls[w, k, 2] + 0.1 - half, walls[w, k, 1], r["pos"][2]]), locked=False)
            ox, oy, _ = scenes.open_spot(walls[w], info[w, 0])
            cx, cy = STRIP * np.clip(np.round(ox / STRIP), -3, 3), STRIP * np.clip(np.round(oy / STRIP), -3, 3)
            for i, s in enumerate(pile):
                r = scenes.slot_record(rec[w], s)
                d = np.zeros(3) if i == 0 else np.append(rng.uniform(-1.2, 1.2, 2), rng.uniform(0.0, 2.0))
                rot = (1, 0, 0, 0) if i == 0 else np.float32(scenes.random_quats(rng, 1)[0])
                scenes.put(r, np.float32([cx + d[0], cy + d[1], r["pos"][2] + d[2]]), rot, locked=(i == 1))
            n = int(rec[w]["nh"] + rec[w]["ns"])
            for i in range(n):
                a = 2 * np.pi * i / n
                r = rec[w]["agents"][i]
                scenes.put(r, np.float32([cx + 0.8 * np.cos(a), cy + 0.8 * np.sin(a), r["pos"][2]]), np.float32(scenes.yaw_quat(a)))
            roles.append(dict(long_box=long_box, far=far, near=near, centre=pile[0], corner=(cx, cy)))
    return edit


def candidates(bodies, meta, walls, info):
    """From a debug dump, float64, per world: wall candidates {slot: [wall indices]} of the dynamic bodies and body-body
    candidates [(a, b)], a < b: AABBs that overlap by more than MARGIN (walls span z in [0, 2.5])."""
    lo, hi = scenes.aabbs(bodies, meta)
    out = []
    for w in range(len(bodies)):
        live = [s for s in range(scenes.SLOTS) if meta[w, s, 0] >= 0]
        dyn = {s: meta[w, s, 1] == 0 for s in live}
        wc = {}
        for s in live:
            if dyn[s] and lo[w, s, 2] <= scenes.WALL_TOP and hi[w, s, 2] >= 0:
                k = walls[w, :info[w, 0]].astype(np.float64)
                hit = ((lo[w, s, 0] + MARGIN <= k[:, 0] + k[:, 2]) & (k[:, 0] - k[:, 2] + MARGIN <= hi[w, s, 0]) &
                       (lo[w, s, 1] + MARGIN <= k[:, 1] + k[:, 3]) & (k[:, 1] - k[:, 3] + MARGIN <= hi[w, s, 1]))
                wc[s] = np.flatnonzero(hit).tolist()
        dd = [(a, b) for i, a in enumerate(live) for b in live[i + 1:] if (dyn[a] or dyn[b]) and
              (lo[w, a] + MARGIN <= hi[w, b]).all() and (lo[w, b] + MARGIN <= hi[w, a]).all()]
        out.append((wc, dd, lo[w], hi[w]))
    return out


def assert_crafted(side, roles):
    """What the crafted scene claims, for every world, from one side's dumps."""
    bodies, meta = side.bodies()
    walls, info = side.walls()
    stats = []
    for w, (wc, dd, lo, hi) in enumerate(candidates(bodies, meta, walls, info)):
        r = roles[w]
        outside = lambda s: (lo[s, :2] > 3 * STRIP).any() or (hi[s, :2] < -3 * STRIP).any()   # beyond an outermost boundary
        assert np.abs(np.r_[lo[r["far"], :2], hi[r["far"], :2]]).min() > 20 and wc[r["far"]] == [], (w, "far body")
        assert outside(r["near"]) and len(wc[r["near"]]) >= 1, (w, "body in an end strip at a wall", wc[r["near"]])
        lb = r["long_box"]
        strips = [int(np.floor(hi[lb, a] / STRIP)) - int(np.floor(lo[lb, a] / STRIP)) + 1 for a in (0, 1)]
        assert min(strips) >= 2 and len(wc[lb]) >= 2, (w, "long box", strips, wc[lb])
        assert tuple(bodies[w, r["centre"], :2]) == r["corner"] and r["corner"][0] % STRIP == 0 and r["corner"][1] % STRIP == 0
        wrapped = [(a, b) for a, b in dd if b - a > 8]
        assert wrapped, (w, "no candidate pair more than 8 slots apart")
        assert len(dd) > DD_CAPACITY, (w, "pile within the LDS capacity", len(dd))
        stats.append((len(dd), len(wrapped), sum(map(len, wc.values()))))
    print("per world (body pairs, of them > 8 slots apart, wall pairs):", stats)


@pytest.mark.parametrize("teams", sorted(TEAMS))
def test_crafted_broadphase_scene_is_not_vacuous_on_the_oracle(oracle, teams):
    """No GPU: after the load every world has a body far outside the walls without a wall candidate, a body beyond the
    last strip boundary with one, the long box across two strips in x and in y with two wall candidates, a body centred
    on a strip corner, a candidate pair more than 8 slots apart and more body pairs than the LDS capacity."""
    hiders, seekers = TEAMS[teams]
    ref = lockstep.make_ref(WORLDS, 0, SEED, hiders, seekers)
    ref.init()
    roles = []
    scenes.inject_ref(ref, crafted_editor(*ref.walls(), roles))
    assert_crafted(ref, roles)


@pytest.mark.gpu
@pytest.mark.parametrize("teams", sorted(TEAMS))
def test_crafted_broadphase_scene_matches_the_oracle(oracle, teams):
    """9 worlds, 8 steps with every action live, every exported tensor, bodies and walls bit for bit after each step;
    body-body pairs spilled beyond the LDS capacity and none dropped."""
    hiders, seekers = TEAMS[teams]
    p = lockstep.Pair(WORLDS, 0, SEED, hiders, seekers)
    roles = []
    scenes.inject(p, crafted_editor(*p.ref.walls(), roles))
    assert_crafted(p.ref, roles)
    p.drive(STEPS, "full")
    st = p.sim.device_status()
    assert st["spilled_dd_pairs"] > 0 and st["dropped_candidate_pairs"] == 0, st


# ------------------------------------------------------------------------------------------------ wall counts
WALLS = dict(worlds=8, seed=0, world_offset=52120)      # found by scanning the oracle's levels on the CPU


def assert_wall_counts(side):
    n = side.walls()[1][:, 0]
    assert n.max() >= 31 and n.min() <= 8, n
    return n


def test_wall_count_scene_is_not_vacuous_on_the_oracle(oracle):
    """No GPU: the octet holds a world with 31 walls (the most that 200 000 generated worlds showed: all but one of
    the staged rows in use) beside one with 8, and bodies touch walls in it during the run."""
    ref = lockstep.make_ref(WALLS["worlds"], 0, WALLS["seed"], world_offset=WALLS["world_offset"])
    ref.init()
    print("walls per world:", assert_wall_counts(ref).tolist())
    draw, cols = lockstep.stream("bench")
    touched = 0
    for s in range(STEPS):
        ref.tensor("action")[:, list(cols)] = draw(s, ref.N * ref.A)
        ref.step()
        touched += sum(len(k) for wc, _, _, _ in candidates(*ref.bodies(), *ref.walls()) for k in wc.values())
    assert touched > 0


@pytest.mark.gpu
def test_wall_count_scene_matches_the_oracle(oracle):
    """8 worlds with 8 .. 31 walls, 8 steps under the benchmark's action stream, bit for bit after each."""
    p = lockstep.Pair(WALLS["worlds"], 0, WALLS["seed"], world_offset=WALLS["world_offset"])
    assert_wall_counts(p.ref)
    p.drive(STEPS, "bench")
    assert p.sim.device_status()["dropped_candidate_pairs"] == 0
