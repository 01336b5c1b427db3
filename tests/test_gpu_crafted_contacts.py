"""Tilted hulls on the floor and against walls, and dense piles, on the device.  The level generator puts every box and
ramp flat on the floor with a yaw only, so the hull-versus-plane contacts of a tilted wedge or box, a tilted hull
against a wall, and more candidate pairs than a world keeps in LDS are met only by accident in the driven parity runs.
Here such scenes are written through the Checkpoint record (oracle/scenes.py) and stepped in lock step with the
oracle, bit for bit.  Agents keep yaw-only poses: the engine never tilts them."""
import numpy as np
import pytest

import lockstep
import scenes

G_DT = 9.8 / 30.0            # what gravity adds to the downward speed of a free body in one step
# A body counts as touched in step 1 when its linear velocity differs from free fall by more than 1e-2 m/s.  Free
# fall itself is off by rounding only: the solver takes velocities from float32 pose differences over h = 1/120 s,
# i.e. 2^-24 x 20 m x 120 / s = 1.4e-4 m/s at the arena's edge; a contact that removes a few centimetres of penetration
# in a substep changes the velocity by metres per second.
TOUCHED = 1e-2


# ------------------------------------------------------------------------------------------------ floor and walls
FLOOR = dict(worlds=256, seed=9)


def floor_editor(walls, info, out):
    """Every box and ramp: a uniformly random rotation; a height that puts its lowest vertex (float64, from the vertex
    set) between 0.3 m below and 0.05 m above the floor; every third one next to a wall, overlapping the wall's box by
    up to 0.3 m; one in five locked; half of the others moving (up to 3 m/s, 2 rad/s).  `out` receives the dynamic ones
    as (world, slot, lin)."""
    def edit(rec, meta):
        rng = np.random.default_rng(77)
        count = 0
        for w in range(len(rec)):
            for s in range(scenes.AGENT_SLOT0):
                kind = int(meta[w, s, 0])
                if kind not in (scenes.CUBE, scenes.BOX, scenes.RAMP):
                    continue
                r = scenes.slot_record(rec[w], s)
                q = np.float32(scenes.random_quats(rng, 1)[0])
                v = scenes.hull_vertices(kind, (0, 0, 0), q)
                pos = np.array(r["pos"], np.float64)
                pos[2] = rng.uniform(-0.3, 0.05) - v[:, 2].min()
                if count % 3 == 0:
                    k = int(rng.integers(0, info[w, 0]))
                    cx, cy, hx, hy = (float(c) for c in walls[w, k])
                    ax = int(rng.integers(0, 2))                      # the wall face whose normal is +-x or +-y ...
                    c, h = ((cx, hx), (cy, hy))[ax]
                    sign = -1.0 if c > 0 else 1.0                      # ... on the side of the arena's centre
                    reach = -(v[:, ax] * sign).min()                   # how far the hull reaches back towards the wall
                    pos[ax] = c + sign * (h + reach - rng.uniform(0.0, 0.3))
                    c2, h2 = ((cy, hy), (cx, hx))[ax]
                    pos[1 - ax] = c2 + rng.uniform(-h2, h2)
                locked = count % 5 == 0
                u, a = rng.normal(size=3), rng.normal(size=3)
                lin = u / np.linalg.norm(u) * rng.uniform(0, 3)
                ang = a / np.linalg.norm(a) * rng.uniform(0, 2)
                if locked or count % 2 == 0:
                    lin = ang = np.zeros(3)
                scenes.put(r, np.float32(pos), q, np.float32(lin), np.float32(ang), locked=locked)
                if not locked:
                    out.append((w, s, np.float32(lin)))
                count += 1
    return edit


def touched_share(bodies, dynamic):
    """The share of the dynamic bodies whose linear velocity after step 1 is not free fall's."""
    n = 0
    for w, s, lin in dynamic:
        free = lin.astype(np.float64) - (0, 0, G_DT)
        n += np.abs(bodies[w, s, 7:10] - free).max() > TOUCHED
    return n / len(dynamic)


def sane(bodies, meta, tag):
    assert np.isfinite(bodies).all(), tag
    q2 = (bodies[:, :, 3:7].astype(np.float64) ** 2).sum(2)
    assert np.abs(q2[meta[:, :, 0] >= 0] - 1).max() < 1e-3, tag


def test_tilted_floor_and_wall_scene_is_not_vacuous_on_the_oracle(oracle):
    """No GPU: in the crafted scene at least half of the dynamic bodies are touched in step 1."""
    ref = lockstep.make_ref(FLOOR["worlds"], seed=FLOOR["seed"])
    ref.init()
    dynamic = []
    scenes.inject_ref(ref, floor_editor(*ref.walls(), dynamic))
    ref.step()
    share = touched_share(ref.bodies()[0], dynamic)
    print(f"{len(dynamic)} dynamic boxes and ramps, {share:.1%} touched in step 1")
    assert share >= 0.5, share
    sane(*ref.bodies(), "step 1")


@pytest.mark.gpu
def test_tilted_hulls_on_the_floor_and_against_walls(oracle):
    """256 worlds of tilted, sunk, moving and locked hulls: 8 steps under the benchmark's action stream, every exported
    tensor, bodies and walls bit for bit after each; on the oracle side at least half of the dynamic bodies are touched
    in step 1, the state stays finite and |q|^2 within 1e-3 of 1."""
    p = lockstep.Pair(FLOOR["worlds"], seed=FLOOR["seed"])
    dynamic = []
    scenes.inject(p, floor_editor(*p.ref.walls(), dynamic))
    draw, cols = lockstep.stream("bench")
    for s in range(8):
        p.step(draw(s, p.rows), cols)
        p.check(f"step {s + 1}")
        sane(*p.ref.bodies(), f"step {s + 1}")
        if s == 0:
            share = touched_share(p.ref.bodies()[0], dynamic)
            assert share >= 0.5, share
    assert p.sim.device_status()["dropped_candidate_pairs"] == 0


# ------------------------------------------------------------------------------------------------ piles
PILE = dict(worlds=64, seed=6, hiders=(3, 3), seekers=(3, 3))
RADIUS = 3.0


def pile_editor(walls, info):
    """All of a world's boxes and ramps in a ball of radius 3 m (centre 2.5 m up) over the spot farthest from the walls,
    random rotations, centres 1 - 4 m high, at rest; the six agents on a ring of radius 4 m around it, facing inwards."""
    def edit(rec, meta):
        rng = np.random.default_rng(31)
        for w in range(len(rec)):
            cx, cy, _ = scenes.open_spot(walls[w], info[w, 0])
            for s in range(scenes.AGENT_SLOT0):
                if meta[w, s, 0] < 0:
                    continue
                while True:
                    d = rng.uniform(-RADIUS, RADIUS, 3)
                    if np.linalg.norm(d) <= RADIUS and 1.0 <= 2.5 + d[2] <= 4.0:
                        break
                scenes.put(scenes.slot_record(rec[w], s), np.float32([cx + d[0], cy + d[1], 2.5 + d[2]]),
                           np.float32(scenes.random_quats(rng, 1)[0]))
            n = int(rec[w]["nh"] + rec[w]["ns"])
            for i in range(n):
                a = 2 * np.pi * i / n
                x, y = cx + 4.0 * np.cos(a), cy + 4.0 * np.sin(a)
                yaw = np.arctan2(-(cx - x), cy - y)                       # local +y (forward) towards the centre
                scenes.put(rec[w]["agents"][i], np.float32([x, y, rec[w]["agents"][i]["pos"][2]]), np.float32(scenes.yaw_quat(yaw)))
    return edit


def overlapping_pairs(bodies, meta):
    """Per world, the pairs of live bodies whose world AABBs (float64, from the vertex sets) overlap."""
    lo, hi = scenes.aabbs(bodies, meta)
    n = np.zeros(len(bodies), int)
    for i in range(scenes.SLOTS):
        for j in range(i + 1, scenes.SLOTS):
            n += ((lo[:, i] <= hi[:, j]) & (lo[:, j] <= hi[:, i])).all(1)
    return n


def dense_enough(bodies, meta):
    pairs = overlapping_pairs(bodies, meta)
    octets = pairs.reshape(-1, 8).sum(1)
    assert octets.max() > 48, octets
    return pairs, octets


def test_pile_scene_is_dense_on_the_oracle(oracle):
    """No GPU: in the loaded scene some octet of worlds has more than 48 pairs of bodies with overlapping AABBs (more
    than one contact round per substep on the device), and at least two octets' worth of worlds have more than 16 (the
    LDS capacity); the oracle alone keeps the pile finite over the 12 steps."""
    ref = lockstep.make_ref(PILE["worlds"], 0, PILE["seed"], PILE["hiders"], PILE["seekers"])
    ref.init()
    scenes.inject_ref(ref, pile_editor(*ref.walls()))
    pairs, octets = dense_enough(*ref.bodies())
    print(f"overlapping AABB pairs per world {pairs.min()}..{pairs.max()}, per octet {octets.min()}..{octets.max()}")
    assert (pairs > 16).sum() >= 16, pairs
    draw, cols = lockstep.stream("full")
    for s in range(12):
        ref.tensor("action")[:] = draw(s, ref.N * ref.A)
        ref.step()
        sane(*ref.bodies(), f"step {s + 1}")


@pytest.mark.gpu
def test_piles_spill_on_the_normal_library_and_match_the_oracle(oracle):
    """64 worlds of 3 + 3 agents around a pile of every box and ramp: 12 steps with grab and lock live, checked every 2,
    and the agents' 32 x 24 views of the pile (k_render on tilted wedges and boxes seen from close by) after the load and
    at the end.  The ordinary library must have spilled body-body pairs and dropped none."""
    W, H = 32, 24
    p = lockstep.Pair(PILE["worlds"], 0, PILE["seed"], PILE["hiders"], PILE["seekers"], render=(W, H))
    scenes.inject(p, pile_editor(*p.ref.walls()))
    dense_enough(*p.ref.bodies())
    p.sim.render()
    p.check_views(W, H, "views after the load")
    p.drive(12, "full", every=2)
    sane(*p.ref.bodies(), "after 12 steps")
    p.sim.render()
    depth, _ = p.check_views(W, H, "views at the end")
    assert (depth > 0).any()
    st = p.sim.device_status()
    print(f"pile: spilled_dd_pairs {st['spilled_dd_pairs']}, spilled_static_pairs {st['spilled_static_pairs']}, "
          f"dropped {st['dropped_candidate_pairs']}")
    assert st["spilled_dd_pairs"] > 0, st
    assert st["dropped_candidate_pairs"] == 0, st
