"""The box rounds of the separating-axis search (hs_k_physics.h phase_sat, hs_collide.h sat_axes_box) on the device.
A box round takes 32 box-only items of an octet of worlds, two lanes per item; an item is a candidate pair of the
broadphase (two bodies, or a body and a wall, whose AABBs overlap).  The scenes here are written through the Checkpoint
record (oracle/scenes.py) so that the FIRST octet files exactly 31, 32, 33 and 65 box-only items in the first substep —
one round with a free pair of lanes, one full round, two rounds, three rounds with the hand-over to a contact round in
between (the pending list holds 48 pairs) — plus the items of one ramp, so that a wedge round follows the box rounds.
9 worlds: one full octet and one partial.  Every scene is stepped 8 times in lock step with the oracle, bit for bit.

How a scene gets its count.  Every box and ramp is parked 30 m up, 10 m apart, where it meets nothing while it falls for
8 steps.  The agents stay on the floor where the level put them; their candidate pairs (with walls, with each other)
are counted.  Then m boxes of a world are moved into a cluster 14 m up (above the walls: no wall candidates), centres
within 0.7 m of each other along every axis: every box contains the ball of radius 0.75 m around its centre, so any two
AABBs overlap by 0.8 m at least whatever the rotations, and the cluster files m (m - 1) / 2 items.  The cluster sizes are
chosen so that the octet's sum is the target.  The count is then confirmed on the loaded oracle state with float64
AABBs from the vertex sets, and no AABB pair may be closer to touching than 5 mm (a body at rest moves 0.07 mm before
the first broadphase), so the float32 predicates of both sides see the same pairs."""
import functools

import numpy as np
import pytest

import lockstep
import scenes

WORLDS, SEED, STEPS = 9, 0, 8
CLUSTER_Z, PARK_Z = 14.0, 30.0
MARGIN = 5e-3
DD_CAP = 16                                       # body pairs a world keeps in LDS (hs_dev.h): more would spill, not be items
TARGETS = (31, 32, 33, 65)
OFFSETS = [(-0.35, -0.35, -0.35), (0.35, 0.35, 0.35), (0.35, -0.35, 0.35), (-0.35, 0.35, 0.35), (0.35, 0.35, -0.35),
           (-0.35, -0.35, 0.35)]
TIE_OVERLAP = 0.0625


def tri(m):
    return m * (m - 1) // 2


def make_ref():
    ref = lockstep.make_ref(WORLDS, 0, SEED)
    ref.init()
    return ref


def item_counts(bodies, meta, walls, info):
    """Per world: (box-only items, items with a ramp, body pairs) of the state, and the smallest distance of any AABB
    pair from touching.  The broadphase's rule (hs_k_physics.h phase_detect): two live bodies of which one is dynamic;
    a dynamic body and a wall, the wall spanning z in [0, 2.5]."""
    lo, hi = scenes.aabbs(bodies, meta)
    n = len(bodies)
    box, wedge, dd = np.zeros(n, int), np.zeros(n, int), np.zeros(n, int)
    margin = np.inf
    for w in range(n):
        live = [i for i in range(scenes.SLOTS) if meta[w, i, 0] in (scenes.CUBE, scenes.BOX, scenes.RAMP, 4, 5)]
        dyn = {i: meta[w, i, 1] == 0 for i in live}
        for a, i in enumerate(live):
            ramp_i = meta[w, i, 0] == scenes.RAMP
            for j in live[a + 1:]:
                if not (dyn[i] or dyn[j]):
                    continue
                gap = max(np.max(lo[w, i] - hi[w, j]), np.max(lo[w, j] - hi[w, i]))
                margin = min(margin, abs(gap))
                if gap <= 0:
                    dd[w] += 1
                    if ramp_i or meta[w, j, 0] == scenes.RAMP:
                        wedge[w] += 1
                    else:
                        box[w] += 1
            if dyn[i]:
                for k in range(info[w, 0]):
                    cx, cy, hx, hy = (float(c) for c in walls[w, k])
                    gap = max(lo[w, i, 0] - (cx + hx), (cx - hx) - hi[w, i, 0], lo[w, i, 1] - (cy + hy), (cy - hy) - hi[w, i, 1],
                              lo[w, i, 2] - scenes.WALL_TOP, -hi[w, i, 2])
                    margin = min(margin, abs(gap))
                    if gap <= 0:
                        if ramp_i:
                            wedge[w] += 1
                        else:
                            box[w] += 1
    return box, wedge, dd, margin


def park_editor(rec, meta, base=None):
    """Every box and ramp to its parking place.  `base` (a one-element list the first call fills): start from the records
    as first saved, so that the agents stand where the level put them in every scene of a run."""
    if base is not None:
        if base[0] is None:
            base[0] = rec.copy()
        rec[:] = base[0]
    for w in range(len(rec)):
        for s in range(scenes.AGENT_SLOT0):
            if meta[w, s, 0] >= 0:
                scenes.put(scenes.slot_record(rec[w], s), np.float32([-20 + 10 * (s % 5), -10 + 10 * (s // 5), PARK_Z]), locked=False)


@functools.lru_cache(maxsize=None)
def layout():
    """From the oracle alone: the hull kinds [WORLDS, 11], a wall-free spot per world, and the box-only items per world
    that remain when every box and ramp is parked (the agents' pairs)."""
    ref = make_ref()
    scenes.inject_ref(ref, park_editor)
    bodies, meta = ref.bodies()
    walls, info = ref.walls()
    box, wedge, _, margin = item_counts(bodies, meta, walls, info)
    ref.close()
    assert margin > MARGIN and not wedge.any(), (margin, wedge)
    spots = [scenes.open_spot(walls[w], info[w, 0]) for w in range(WORLDS)]
    return meta[:, :scenes.AGENT_SLOT0, 0].copy(), spots, box


@functools.lru_cache(maxsize=None)
def cluster_sizes(target):
    """m[w] for the worlds of the first octet with sum of m (m - 1) / 2 = target - the agents' items, using as many
    worlds as possible.  World 0 also takes a ramp into its cluster, so its body pairs m (m - 1) / 2 + m must fit in LDS."""
    kinds, _, base = layout()
    need = target - int(base[:8].sum())
    caps = []
    for w in range(8):
        have = int(((kinds[w] == scenes.CUBE) | (kinds[w] == scenes.BOX)).sum())
        caps.append(max(m for m in range(len(OFFSETS) + 1) if m <= have and tri(m) + (m if w == 0 else 0) <= DD_CAP))

    @functools.lru_cache(maxsize=None)
    def best(w, left):
        if w == 8:
            return (0, ()) if left == 0 else None
        out = None
        for m in range(caps[w] + 1):
            if m == 1 or tri(m) > left or (w == 0 and m < 2):
                continue
            rest = best(w + 1, left - tri(m))
            if rest is not None and (out is None or rest[0] + (m > 0) > out[0]):
                out = (rest[0] + (m > 0), (m,) + rest[1])
        return out
    found = best(0, need)
    assert found is not None, (target, need, caps)
    return found[1] + (3,)                       # the partial octet: three boxes


def count_editor(target, base=None):
    kinds, spots, _ = layout()
    sizes = cluster_sizes(target)

    def edit(rec, meta):
        park_editor(rec, meta, base)
        rng = np.random.default_rng(500 + target)
        for w in range(WORLDS):
            cx, cy, _ = spots[w]
            slots = [s for s in range(scenes.RAMP_SLOT0) if kinds[w, s] in (scenes.CUBE, scenes.BOX)][:sizes[w]]
            if w == 0:
                slots.append(scenes.RAMP_SLOT0)
            for k, s in enumerate(slots):
                off = (0.0, 0.0, 0.0) if s == scenes.RAMP_SLOT0 else OFFSETS[k]
                # every other cluster keeps yaw-only poses (parallel z axes), the rest tumble
                q = scenes.yaw_quat(rng.uniform(-np.pi, np.pi)) if w % 2 else scenes.random_quats(rng, 1)[0]
                scenes.put(scenes.slot_record(rec[w], s), np.float32([cx + off[0], cy + off[1], CLUSTER_Z + off[2]]), np.float32(q))
    return edit


def tie_editor(rec, meta, base=None):
    """Up to four boxes of every world on the floor around its wall-free spot, axis-aligned (the long ones along x or,
    by a float32 quarter turn, along y), in a 2 x 2 block whose neighbours overlap by 1/16 m: across a side of the
    block two faces tie in z and in the direction along the side, across the diagonal the x and y faces tie with
    each other — on dyadic coordinates exactly, and between the two lanes of a pair (A's best face against B's)."""
    kinds, spots, _ = layout()
    park_editor(rec, meta, base)
    for w in range(len(rec)):
        cx, cy, _ = spots[w]
        slots = [s for s in range(scenes.RAMP_SLOT0) if kinds[w, s] in (scenes.CUBE, scenes.BOX)][:4]
        for k, s in enumerate(slots):
            turn = kinds[w, s] == scenes.BOX and k % 2 == 1
            hx, hy = ((4.0, 0.75) if not turn else (0.75, 4.0)) if kinds[w, s] == scenes.BOX else (1.0, 1.0)
            sx, sy = (-1, 1)[k & 1], (-1, 1)[k >> 1]
            pos = [cx + sx * (hx - TIE_OVERLAP / 2), cy + sy * (hy - TIE_OVERLAP / 2), 1.0]
            scenes.put(scenes.slot_record(rec[w], s), np.float32(pos), np.float32(scenes.yaw_quat(np.pi / 2 if turn else 0.0)))


def first_substep_items(ref):
    box, wedge, dd, margin = item_counts(*ref.bodies(), *ref.walls())
    return box, wedge, dd, margin


@pytest.mark.parametrize("target", TARGETS)
def test_the_scene_files_the_target_count_on_the_oracle(oracle, target):
    """No GPU: in the loaded scene the first octet has exactly `target` box-only items and the items of one ramp, no
    world has more body pairs than LDS holds, and no AABB pair is within 5 mm of touching."""
    ref = make_ref()
    scenes.inject_ref(ref, count_editor(target))
    box, wedge, dd, margin = first_substep_items(ref)
    ref.close()
    print(f"target {target}: clusters {cluster_sizes(target)}, box items per world {box.tolist()}, with a ramp {wedge.tolist()}, "
          f"margin {margin:.4f}")
    assert box[:8].sum() == target and box[8] >= 3, box
    assert wedge[0] >= 2 and not wedge[1:].any(), wedge
    assert dd.max() <= DD_CAP and margin > MARGIN, (dd, margin)


def test_the_tie_scene_ties_on_the_oracle(oracle):
    """No GPU: every world of the tie scene has a diagonal pair of boxes whose overlaps along x and y are the same float32
    number, and side pairs whose overlap is exactly 1/16 m."""
    ref = make_ref()
    scenes.inject_ref(ref, tie_editor)
    bodies, meta = ref.bodies()
    box, _, _, _ = first_substep_items(ref)
    ref.close()
    lo, hi = scenes.aabbs(bodies, meta)
    diagonal = side = 0
    for w in range(WORLDS):
        on_floor = [s for s in range(scenes.RAMP_SLOT0) if meta[w, s, 0] >= 0 and bodies[w, s, 2] == 1.0]
        for a, i in enumerate(on_floor):
            for j in on_floor[a + 1:]:
                over = np.minimum(hi[w, i], hi[w, j]) - np.maximum(lo[w, i], lo[w, j])
                both_exact = (bodies[w, [i, j], 4:7] == 0).all()
                diagonal += over[0] == over[1] == TIE_OVERLAP and both_exact
                side += (over[0] == TIE_OVERLAP) != (over[1] == TIE_OVERLAP) and both_exact
    print(f"tie scene: {diagonal} diagonal ties, {side} side pairs, box items per world {box.tolist()}")
    assert diagonal >= 2 and side >= WORLDS and (box >= 4).all(), (diagonal, side, box)


@pytest.mark.gpu
def test_box_rounds_match_the_oracle(oracle):
    """The four counted scenes and the tie scene one after the other on one pair of 9 worlds: 8 steps each, nobody acts,
    every exported tensor, the bodies and the walls bit for bit after every step; nothing spills and nothing is
    dropped (the items are the candidates)."""
    p = lockstep.Pair(WORLDS, 0, SEED)
    base = [None]
    for name, edit in [(f"{t} items", count_editor(t, base)) for t in TARGETS] + [("ties", lambda r, m: tie_editor(r, m, base))]:
        scenes.inject(p, edit)
        if name != "ties":
            box, wedge, _, margin = first_substep_items(p.ref)
            assert box[:8].sum() == int(name.split()[0]) and wedge[0] >= 2 and margin > MARGIN, (name, box, wedge, margin)
        for s in range(STEPS):
            p.step()
            p.check(f"{name}, step {s + 1}")
        assert np.isfinite(p.ref.bodies()[0]).all(), name
    st = p.sim.device_status()
    assert st["spilled_dd_pairs"] == 0 and st["spilled_static_pairs"] == 0 and st["dropped_candidate_pairs"] == 0, st
    p.sim.close(); p.ref.close()
