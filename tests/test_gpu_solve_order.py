"""The body-body solve order and the manifold record paths of k_physics (hs_k_physics.h phase_dd, wall_round, last_round)
on crafted scenes, written through the Checkpoint record (oracle/scenes.py) and stepped in lock step with the oracle, bit
for bit: a pile with three batches of body-body manifolds in every world, a dependency chain, one box in five manifolds
and a candidate pair that does not collide between accepted ones; and bodies pressed against walls, more colliding pairs
per octet than one contact round takes, so that the records of one substep lie partly in LDS and partly in the global
workspace.  12 worlds: one full octet and one with four padding slots.

What a scene holds is counted from its construction, in float64 and without the device or the oracle's collision code:
every body used here is a box with a yaw-only pose and every wall an axis-aligned box, for which the separating-axis
test over the four face normals in the plane plus the z extents is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

import lockstep
import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLDS, SEED, STEPS = 12, 6, 12
AGENTS6 = dict(hiders=(3, 3), seekers=(3, 3))
HALF = {scenes.CUBE: (1.0, 1.0, 1.0), scenes.BOX: (4.0, 0.75, 1.0), scenes.AGENT_OBJ: (1.0, 1.0, 1.0), 5: (1.0, 1.0, 1.0)}
PRESS = 0.1                   # how far neighbours overlap
CLEAR = 1e-3                  # a pair counts as colliding / separate only when it is so by more than this (metres)
DIAG = float(np.sqrt(2.0))


# ------------------------------------------------------------------------------------------------ float64 geometry
def yaw_of(q):
    return 2.0 * np.arctan2(float(q[3]), float(q[0]))


def box2d(pos, yaw, half):
    """(centre xy, the two face normals, half extents xy, z range) of a yaw-only box."""
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array(pos[:2], np.float64), np.array([[c, s], [-s, c]]), np.array(half[:2], np.float64), \
        (float(pos[2]) - half[2], float(pos[2]) + half[2])


def overlap(a, b):
    """Penetration of two yaw-only boxes, float64: the smallest overlap over the four face normals and z (negative: the
    gap along the best separating axis)."""
    (ca, na, ha, za), (cb, nb, hb, zb) = a, b
    best = min(za[1] - zb[0], zb[1] - za[0])
    for ax in list(na) + list(nb):
        ra = np.abs(na @ ax) @ ha
        rb = np.abs(nb @ ax) @ hb
        best = min(best, ra + rb - abs((cb - ca) @ ax))
    return best


def aabb(box):
    c, n, h, z = box
    r = np.abs(n.T) @ h
    return np.array([c[0] - r[0], c[1] - r[1], z[0]]), np.array([c[0] + r[0], c[1] + r[1], z[1]])


def world_boxes(bodies, meta, w):
    """slot -> box of the yaw-only boxes of world w (ramps are kept out of reach in these scenes), and which are dynamic."""
    out = {}
    for s in range(scenes.SLOTS):
        kind = int(meta[w, s, 0])
        if kind in HALF:
            out[s] = box2d(bodies[w, s, :3], yaw_of(bodies[w, s, 3:7]), HALF[kind])
    return out


def body_pairs(boxes):
    """The body-body candidates (overlapping AABBs) of a world in pair order, as (a, b, penetration)."""
    out = []
    slots = sorted(boxes)
    for i, a in enumerate(slots):
        for b in slots[i + 1:]:
            (la, ha), (lb, hb) = aabb(boxes[a]), aabb(boxes[b])
            if (la <= hb).all() and (lb <= ha).all():
                out.append((a, b, overlap(boxes[a], boxes[b])))
    return out


def wall_pairs(boxes, walls, count):
    out = []
    for s in sorted(boxes):
        for k in range(count):
            cx, cy, hx, hy = (float(v) for v in walls[k])
            d = overlap(boxes[s], box2d((cx, cy, scenes.WALL_TOP / 2), 0.0, (hx, hy, scenes.WALL_TOP / 2)))
            if d > CLEAR:
                out.append((s, k, d))
    return out


def chain_depth(accepted):
    """Rounds a world's accepted manifolds need when each waits for every earlier one that shares a body with it."""
    level = []
    for i, (a, b) in enumerate(accepted):
        level.append(1 + max([level[j] for j in range(i) if {a, b} & set(accepted[j])], default=0))
    return max(level, default=0)


# ------------------------------------------------------------------------------------------------ the scenes
def live(meta, w, kinds):
    return [s for s in range(scenes.AGENT_SLOT0) if int(meta[w, s, 0]) in kinds]


def park(rec, meta, w, used):
    """Everything the scene does not use (ramps, further boxes): in the air, 4 m apart, out of every wall's z range."""
    for s in range(scenes.AGENT_SLOT0):
        if meta[w, s, 0] >= 0 and s not in used:
            scenes.put(scenes.slot_record(rec[w], s), np.float32([0.0, 0.0, 30.0 + 4.0 * s]), np.float32([1, 0, 0, 0]))


def pile_editor(walls, info):
    """Per world, around the spot farthest from the walls, all at rest on the floor: long box E0 along x; the first cube
    and agents 0-2 in a row along its +y side, each pressed 0.1 m into E0 and into its neighbour; long boxes E1 and E2
    pressed against its -y side one behind the other; agent 3, turned by 45 degrees, with a corner 0.1 m inside the +x end
    of E2 — its AABB overlaps E1's, the hulls are 0.5 m apart.  Agents 4 and 5 (where they exist) form a second row
    behind agents 0 and 1."""
    def edit(rec, meta):
        for w in range(len(rec)):
            cx, cy, _ = scenes.open_spot(walls[w], info[w, 0])
            longs, cubes = live(meta, w, (scenes.BOX,))[:3], live(meta, w, (scenes.CUBE,))[:1]
            assert len(longs) == 3 and len(cubes) == 1, "every level has three long boxes and a cube"
            park(rec, meta, w, longs + cubes)
            flat = np.float32([1, 0, 0, 0])
            for i, s in enumerate(longs):
                y = -i * (0.75 + 0.75 - PRESS)
                scenes.put(scenes.slot_record(rec[w], s), np.float32([cx, cy + y, 1.0]), flat)
            row = 0.75 + 1.0 - PRESS
            scenes.put(scenes.slot_record(rec[w], cubes[0]), np.float32([cx - 2.9, cy + row, 1.0]), flat)
            n = int(rec[w]["nh"] + rec[w]["ns"])
            for i in range(n):
                a = rec[w]["agents"][i]
                z = a["pos"][2]
                if i < 3:
                    scenes.put(a, np.float32([cx - 2.9 + 1.9 * (i + 1), cy + row, z]), flat)
                elif i == 3:
                    y = -2 * (0.75 + 0.75 - PRESS)
                    scenes.put(a, np.float32([cx + 4.0 + DIAG - PRESS, cy + y, z]), np.float32(scenes.yaw_quat(np.pi / 4)))
                else:
                    scenes.put(a, np.float32([cx - 2.9 + 1.9 * (i - 3), cy + row + 1.9, z]), flat)
    return edit


def wall_editor(walls, info):
    """Per world the three long boxes, the first cube and every agent, each pressed 0.2 m into a wall of its own from the
    side of the arena's centre, the long boxes along their wall."""
    def edit(rec, meta):
        for w in range(len(rec)):
            longs, cubes = live(meta, w, (scenes.BOX,))[:3], live(meta, w, (scenes.CUBE,))[:1]
            park(rec, meta, w, longs + cubes)
            n = int(rec[w]["nh"] + rec[w]["ns"])
            bodies = [(scenes.slot_record(rec[w], s), HALF[int(meta[w, s, 0])]) for s in longs + cubes]
            bodies += [(rec[w]["agents"][i], HALF[scenes.AGENT_OBJ]) for i in range(n)]
            nw = int(info[w, 0])
            for i, (r, half) in enumerate(bodies):
                cx, cy, hx, hy = (float(c) for c in walls[w, (i * 3 + w) % nw])
                along_x = hx >= hy                                   # the wall's long side
                c, h = (cy, hy) if along_x else (cx, hx)
                sign = -1.0 if c > 0 else 1.0                        # the face on the side of the arena's centre
                reach = half[1] if half[0] > half[1] else half[0]    # a long box lies along the wall
                off = c + sign * (h + reach - 0.2)
                pos = [cx, off] if along_x else [off, cy]
                yaw = 0.0 if along_x or half[0] == half[1] else np.pi / 2
                scenes.put(r, np.float32(pos + [float(r["pos"][2]) if i >= 4 else 1.0]), np.float32(scenes.yaw_quat(yaw)))
    return edit


def census(bodies, meta, walls, info):
    """Per world: the accepted body-body pairs in pair order, the candidates that are not accepted, the wall pairs."""
    out = []
    for w in range(len(bodies)):
        boxes = world_boxes(bodies, meta, w)
        cand = body_pairs(boxes)
        assert all(abs(d) > CLEAR for _, _, d in cand), ("a pair within rounding of touching", w, cand)
        acc = [(a, b) for a, b, d in cand if d > 0]
        gaps = [k for k, (_, _, d) in enumerate(cand) if d < 0]
        out.append(dict(cand=[(a, b) for a, b, _ in cand], acc=acc, gaps=gaps, walls=wall_pairs(boxes, walls[w], int(info[w, 0]))))
    return out


def check_pile(cs, agents):
    for w, c in enumerate(cs):
        acc, cand = c["acc"], c["cand"]
        assert len(acc) >= 9 and (len(acc) + 3) // 4 >= 3, (w, acc)            # three batches of four
        assert chain_depth(acc) >= 4, (w, acc)
        count = {}
        for a, b in acc:
            count[a] = count.get(a, 0) + 1; count[b] = count.get(b, 0) + 1
        assert max(v for s, v in count.items() if s < scenes.AGENT_SLOT0) >= 4, (w, count)     # one BOX in four manifolds
        # a candidate that does not collide, with accepted ones before and after it in candidate order
        assert any(min(cand.index(p) for p in acc) < k < max(cand.index(p) for p in acc) for k in c["gaps"]), (w, cand, acc)
    return min(len(c["acc"]) for c in cs), max(len(c["cand"]) for c in cs)


def check_walls(cs):
    per_octet = [sum(len(c["acc"]) + len(c["walls"]) for c in cs[o:o + 8]) for o in range(0, len(cs), 8)]
    assert max(per_octet) > 48, per_octet                                       # more than one contact round can hold
    return per_octet


def sane(bodies, meta, tag):
    assert np.isfinite(bodies).all(), tag
    q2 = (bodies[:, :, 3:7].astype(np.float64) ** 2).sum(2)
    assert np.abs(q2[meta[:, :, 0] >= 0] - 1).max() < 1e-3, tag


@pytest.mark.parametrize("agents", [{}, AGENTS6], ids=["4 agents", "6 agents"])
def test_scenes_are_not_vacuous_on_the_oracle(oracle, agents):
    """No GPU.  Pile: every world has at least nine accepted body-body manifolds (three batches), a dependency chain at
    least four deep, a box in at least four manifolds and a non-colliding candidate between accepted ones.  Walls: an
    octet has more than 48 colliding pairs.  The oracle keeps both finite over the 12 steps, and in step 1 every body
    of an accepted pair of the pile is moved by its contacts."""
    ref = lockstep.make_ref(WORLDS, 0, SEED, **agents)
    ref.init()
    scenes.inject_ref(ref, pile_editor(*ref.walls()))
    cs = census(*ref.bodies(), *ref.walls())
    least, most = check_pile(cs, agents)
    print(f"pile: accepted body-body manifolds per world >= {least}, candidates <= {most}")
    before = ref.bodies()[0].copy()
    draw, cols = lockstep.stream("full")
    for s in range(STEPS):
        ref.tensor("action")[:] = draw(s, ref.N * ref.A)
        ref.step()
        sane(*ref.bodies(), f"pile step {s + 1}")
        if s == 0:
            moved = np.abs(ref.bodies()[0][:, :, :2] - before[:, :, :2]).max(2) > 1e-3     # pressed 0.1 m: pushed apart
            for w, c in enumerate(cs):
                assert all(moved[w, a] or moved[w, b] for a, b in c["acc"]), (w, c["acc"], moved[w])
    ref = lockstep.make_ref(WORLDS, 0, SEED, **agents)
    ref.init()
    scenes.inject_ref(ref, wall_editor(*ref.walls()))
    per_octet = check_walls(census(*ref.bodies(), *ref.walls()))
    print(f"walls: colliding pairs per octet {per_octet}")
    for s in range(STEPS):
        ref.tensor("action")[:] = draw(s, ref.N * ref.A)
        ref.step()
        sane(*ref.bodies(), f"walls step {s + 1}")


def run_scene(editor, agents, check):
    """12 lock steps (48 substeps) of the scene under the full action stream, everything compared after every step."""
    p = lockstep.Pair(WORLDS, 0, SEED, **agents)
    scenes.inject(p, editor(*p.ref.walls()))
    check(census(*p.ref.bodies(), *p.ref.walls()))
    p.drive(STEPS, "full", every=1)
    sane(*p.ref.bodies(), "after 12 steps")
    st = p.sim.device_status()
    assert st["dropped_candidate_pairs"] == 0, st
    return st


@pytest.mark.gpu
def test_pile_in_three_batches_matches_the_oracle(oracle):
    run_scene(pile_editor, {}, lambda cs: check_pile(cs, {}))


@pytest.mark.gpu
def test_pile_with_six_agents_matches_the_oracle(oracle):
    """k_physics<3>: 17 body slots, three rounds of bodies."""
    run_scene(pile_editor, AGENTS6, lambda cs: check_pile(cs, AGENTS6))


@pytest.mark.gpu
def test_bodies_pressed_against_walls_match_the_oracle(oracle):
    """More than 48 colliding pairs in an octet: the manifolds of the first contact round go to the global workspace,
    those of the last stay in LDS, and the solver reads and writes both in one substep."""
    run_scene(wall_editor, {}, check_walls)


CHILD = """
import sys
for p in %r:
    sys.path.insert(0, p)
import hs_ref
hs_ref.build()
import test_gpu_solve_order as t
st = t.run_scene(t.pile_editor, {}, lambda cs: t.check_pile(cs, {}))
print("SPILLED", st["spilled_dd_pairs"], st["spilled_static_pairs"])
"""


@pytest.mark.gpu
def test_pile_through_the_small_capacities_matches_the_oracle(oracle):
    """The pile on the build whose LDS capacities are one pair of each kind: every manifold but the first of a world goes
    through the workspace and the spill path.  (A child process, so that HS_LIB_PATH can select the library.)"""
    import build as hs_build
    paths = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "marl-hideandseek_amd")]
    out = subprocess.run([sys.executable, "-c", CHILD % (paths,)], env={**os.environ, "HS_LIB_PATH": hs_build.build_smallcap()},
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    spilled = [l for l in out.stdout.splitlines() if l.startswith("SPILLED")][0].split()
    assert int(spilled[1]) > 0 and int(spilled[2]) >= 0, out.stdout
