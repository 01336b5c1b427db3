"""The stored narrowphase cases on the device.  tests/golden/narrowphase_cases.npz holds 1 200 random hull pairs (half of
them fully random rotations, all three hull kinds) whose oracle manifolds test_oracle_first_principles.py pins against
a linear program.  Here every one of them is written into a training world through the Checkpoint record
(oracle/scenes.py), 14 m above a wall-free spot where nothing else is, and the kernel's integrate -> broadphase ->
narrowphase -> solve on these poses is compared with the oracle's bit for bit: at rest, and with random velocities and
locked bodies; through the normal library and, in a child process, through the small-capacity build's spill path."""
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import lockstep
import scenes
from scenes import BOX, CUBE, RAMP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "marl-hideandseek_amd")
CASES = os.path.join(ROOT, "tests", "golden", "narrowphase_cases.npz")

WORLDS, SEED, HEIGHT = 512, 2, 14.0          # one stored pair per world; seed 2 has enough worlds with two cubes
KINDS = (CUBE, RAMP, BOX)
COMBOS = [(a, b) for i, a in enumerate(KINDS) for b in KINDS[i:]]      # the six unordered kind combinations


@functools.lru_cache(maxsize=None)
def stored():
    g = np.load(CASES)["cases"]
    assert g.shape == (1200, 20)
    return g


def batches():
    n = len(stored())
    return [np.arange(lo, min(lo + WORLDS, n)) for lo in range(0, n, WORLDS)]


def make_ref():
    ref = lockstep.make_ref(WORLDS, flags=0, seed=SEED)
    ref.init()
    return ref


@functools.lru_cache(maxsize=None)
def layout():
    """What the level generator gives: the hull kind of every box / ramp slot [WORLDS, 11] and a wall-free (x, y) per
    world (the spot farthest from every wall).  A load regenerates the same level from the record's key."""
    ref = make_ref()
    kinds = ref.bodies()[1][:, :scenes.AGENT_SLOT0, 0].copy()
    walls, info = ref.walls()
    spots = np.array([scenes.open_spot(walls[w], info[w, 0])[:2] for w in range(WORLDS)])
    ref.close()
    assert ((kinds == BOX).sum(1) >= 2).all() and ((kinds == RAMP).sum(1) == 2).all()
    return kinds, spots


@functools.lru_cache(maxsize=None)
def placement(batch):
    """[(row, world, slot of A, slot of B)] for the rows of one batch: the rows that need the most cubes get the worlds
    that have the most."""
    kinds, _ = layout()
    rows = batches()[batch]
    g = stored()
    need = np.array([int(g[r, 0] == CUBE) + int(g[r, 1] == CUBE) for r in rows])
    worlds = np.argsort(-(kinds == CUBE).sum(1), kind="stable")
    out = []
    for r, w in zip(rows[np.argsort(-need, kind="stable")], worlds):
        oa, ob = int(g[r, 0]), int(g[r, 1])
        sa = int(np.flatnonzero(kinds[w] == oa)[0]) if (kinds[w] == oa).any() else -1
        cand = [int(s) for s in np.flatnonzero(kinds[w] == ob) if s != sa]
        assert sa >= 0 and cand, f"no world left with the hulls of stored row {r}: kinds {oa}, {ob}"
        out.append((int(r), int(w), sa, cand[0]))
    return sorted(out)


def editor(batch, motion, only=None, base=None):
    """edit(records, meta) that writes the batch's stored poses, translated by the world's offset, into the records as
    first saved (`base`, a one-element list the first call fills): every other body stays where the level put it.
    `only` = 0 / 1 places only body A / B (the free-fall controls).  `motion`: seeded velocities up to 3 m/s and
    2 rad/s, and one body in four locked (a locked body is at rest)."""
    g = stored()
    _, spots = layout()
    base = [None] if base is None else base

    def edit(rec, meta):
        if base[0] is None:
            base[0] = rec.copy()
        rec[:] = base[0]
        rng = np.random.default_rng(1000 + batch)
        for r, w, sa, sb in placement(batch):
            assert meta[w, sa, 0] == g[r, 0] and meta[w, sb, 0] == g[r, 1]
            off = np.array([spots[w, 0], spots[w, 1], HEIGHT])
            for k, (slot, pos, rot) in enumerate(((sa, g[r, 2:5], g[r, 5:9]), (sb, g[r, 9:12], g[r, 12:16]))):
                u, v = rng.normal(size=3), rng.normal(size=3)
                lin = u / np.linalg.norm(u) * rng.uniform(0, 3)
                ang = v / np.linalg.norm(v) * rng.uniform(0, 2)
                locked = rng.random() < 0.25
                if only is not None and k != only:
                    continue
                if not motion:
                    lin = ang = np.zeros(3); locked = False
                elif locked:
                    lin = ang = np.zeros(3)
                scenes.put(scenes.slot_record(rec[w], slot), np.float32(pos + off), np.float32(rot), np.float32(lin),
                           np.float32(ang), locked=locked)
    return edit


@functools.lru_cache(maxsize=None)
def collided(batch):
    """Oracle side only: per placed row, whether either body's linear velocity after step 1 differs (bitwise) from its
    free fall — the same step of the same loaded state without the other body of the pair."""
    lin = []
    ref = make_ref()
    base = [None]
    for only in (None, 0, 1):
        scenes.inject_ref(ref, editor(batch, False, only, base))
        ref.step()
        lin.append(lockstep.bits(ref.bodies()[0][:, :, 7:10]).copy())
    ref.close()
    full, a_alone, b_alone = lin
    return np.array([not (np.array_equal(full[w, sa], a_alone[w, sa]) and np.array_equal(full[w, sb], b_alone[w, sb]))
                     for _, w, sa, sb in placement(batch)])


def combo(r):
    a, b = int(stored()[r, 0]), int(stored()[r, 1])
    return (a, b) if KINDS.index(a) <= KINDS.index(b) else (b, a)


def run(motion, which):
    """Lock-step run of the batches `which` on one Pair: check after the load and after every checked step.  Returns
    (sha256 of the GPU body state at the checked steps, rows placed, device status)."""
    p = lockstep.Pair(WORLDS, flags=0, seed=SEED)
    checked = (2, 4, 6) if motion else (1, 4)
    h = hashlib.sha256()
    base, placed = [None], 0
    for b in which:
        scenes.inject(p, editor(b, motion, base=base))
        placed += len(placement(b))
        for s in range(1, checked[-1] + 1):
            p.step()
            if s in checked:
                p.check(f"batch {b} step {s}")
                h.update(p.sim.debug_bodies()[0].tobytes())
    st = p.sim.device_status()
    p.sim.close(); p.ref.close()
    return h.hexdigest(), placed, st


@functools.lru_cache(maxsize=None)
def normal_run_of_first_batch(motion):
    return run(motion, [0])


def test_the_placement_is_not_vacuous_on_the_oracle(oracle):
    """No GPU: every stored row gets a world, and on the oracle alone at least 150 placed pairs collide in step 1 and at
    least 150 do not (the bounds the stored test asserts on the untranslated poses), with at least one colliding pair
    of each of the six kind combinations, ramp-ramp included."""
    rows = [r for b in range(len(batches())) for r, _, _, _ in placement(b)]
    assert sorted(rows) == list(range(len(stored())))
    hit = np.concatenate([collided(b) for b in range(len(batches()))])
    per = {c: int(sum(h for r, h in zip(rows, hit) if combo(r) == c)) for c in COMBOS}
    print(f"collided {int(hit.sum())}, not collided {int((~hit).sum())}, per kind pair {per}")
    assert hit.sum() >= 150 and (~hit).sum() >= 150, (hit.sum(), (~hit).sum())
    assert all(v >= 1 for v in per.values()), per


@pytest.mark.gpu
@pytest.mark.parametrize("motion", [False, True], ids=["at_rest", "moving"])
def test_stored_pairs_match_the_oracle(oracle, motion):
    """All 1 200 stored pairs in three batches on one Pair, bit for bit against the oracle: every exported tensor, bodies
    and walls after the load, after steps 1 and 4 (at rest) or every 2 of 6 steps (moving).  Nobody acts."""
    first = normal_run_of_first_batch(motion)
    rest = run(motion, range(1, len(batches())))
    assert first[1] + rest[1] == len(stored()), "every stored case is placed"
    assert first[2]["dropped_candidate_pairs"] == 0 and rest[2]["dropped_candidate_pairs"] == 0
    if not motion:
        hit = np.concatenate([collided(b) for b in range(len(batches()))])
        rows = [r for b in range(len(batches())) for r, _, _, _ in placement(b)]
        assert hit.sum() >= 150 and (~hit).sum() >= 150, (hit.sum(), (~hit).sum())
        for c in COMBOS:
            assert any(h for r, h in zip(rows, hit) if combo(r) == c), f"no colliding pair of kinds {c}"


CHILD = """
import sys
for p in {paths!r}:
    sys.path.insert(0, p)
import hs_ref
hs_ref.build()
import test_gpu_crafted_narrowphase as t
digest, placed, st = t.run({motion!r}, [0])
print("CRAFTED", digest, placed, st["spilled_dd_pairs"], st["dropped_candidate_pairs"])
"""


@pytest.mark.gpu
@pytest.mark.parametrize("motion", [False, True], ids=["at_rest", "moving"])
def test_stored_pairs_through_the_spill_path(oracle, motion):
    """The first batch through libhideseek_smallcap.so (capacities of one pair: nearly every candidate pair spills), in a
    child process because the library is chosen at import: same oracle parity, pairs spilled, none dropped, and the
    body-state digest of the normal library on that batch."""
    import build as hs_build
    code = CHILD.format(paths=[PKG, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")], motion=motion)
    out = subprocess.run([sys.executable, "-c", code], env={**os.environ, "HS_LIB_PATH": hs_build.build_smallcap()},
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    small = [l for l in out.stdout.splitlines() if l.startswith("CRAFTED")][0].split()
    assert int(small[2]) == WORLDS and int(small[3]) > 0 and small[4] == "0", small
    normal = normal_run_of_first_batch(motion)
    assert normal[0] == small[1], "same trajectory whichever path a pair takes"
