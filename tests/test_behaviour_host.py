"""The contract of hs_behaviour_stats (include/hideseek.h) restated in numpy, one float32 operation at a time, and what can
be checked of it without a GPU: properties of the restatement on hand-written inputs, gpu_hideseek.behaviour.eager_step
against it, the refusals of gpu_hideseek.behaviour.request, stats_to_metrics with zero counts and the agreement of the
ctypes mirror with the header.  tests/test_gpu_behaviour.py compares the kernel with behaviour_step bit for bit on inputs
made here and on the simulator's own exports."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, I = np.float32, np.int32
STATS, KIND, SIDE = 27, 9, 3
UNARMED, PREP, MAIN, WAITING = 0, 1, 2, 3
WORLD_EPISODES, REACHED_MAIN, BAD, BOXES, RAMPS, SEEKERS, HIDERS = 0, 1, 2, 3, 12, 21, 24
MAX_PREP, MAX_MAIN, MOVED_PREP, MOVED_MAIN, HID_PREP, SEEK_PREP, HID_END, SEEK_END, OBJECTS = range(9)
F32_SUMS = (BOXES + MAX_PREP, BOXES + MAX_MAIN, RAMPS + MAX_PREP, RAMPS + MAX_MAIN, SEEKERS, HIDERS)      # the others are sums of integers
EPS = 0.5
WORLD_KEYS = ("phase", "n_obj", "n_side", "start_pos", "prep_pos", "last_pos", "prep_locks", "last_locks", "travel", "grab", "agent_steps")
ROW_KEYS = ("was_active",)
INPUTS = ("positions", "locks", "counts", "prep_counter", "done", "self_type", "self_mask", "grabbing")


def new_state(worlds, A, phase=UNARMED):
    return dict(phase=np.full(worlds, phase, I), n_obj=np.zeros((worlds, 2), I), n_side=np.zeros((worlds, 2), I), start_pos=np.zeros((worlds, 11, 2), F),
                prep_pos=np.zeros((worlds, 11, 2), F), last_pos=np.zeros((worlds, 17, 2), F), prep_locks=np.zeros((worlds, 11), I),
                last_locks=np.zeros((worlds, 11), I), travel=np.zeros((worlds, 2), F), grab=np.zeros((worlds, 2), I), agent_steps=np.zeros((worlds, 2), I),
                was_active=np.zeros(worlds * A, I))


def dist(a, b):
    """d(a, b) of the contract: every operation rounded to float32 on its own."""
    dx, dy = F(a[0] - b[0]), F(a[1] - b[1])
    xx, yy = F(dx * dx), F(dy * dy)
    return np.sqrt(F(xx + yy))


def behaviour_step(st, table, A, positions, locks, counts, prep_counter, done, self_type, self_mask, grabbing, move_eps=EPS, booked=None):
    """The contract, world by world in the header's order; `st` (new_state) is updated in place, `table` [27] f64 is added
    to in world order.  `booked`, if given, is {table index: list} and receives the f32-valued terms (maxima, travel) of
    the episodes that end, for the bound on their sums."""
    worlds = st["phase"].shape[0]
    positions = np.asarray(positions, F).reshape(worlds, 17, 2)
    locks, counts = np.asarray(locks, I).reshape(worlds, 11), np.asarray(counts, I).reshape(worlds, 4)
    prep_counter, done, self_type = (np.asarray(x).reshape(worlds, A) for x in (prep_counter, done, self_type))
    self_mask, grabbing = np.asarray(self_mask, F).reshape(worlds, A), np.asarray(grabbing, F).reshape(worlds, A)
    was = st["was_active"].reshape(worlds, A)
    eps = F(move_eps)

    def add(i, v):
        table[i] += float(v)
        if booked is not None and i in F32_SUMS:
            booked.setdefault(i, []).append(float(v))
    with np.errstate(all="ignore"):
        for w in range(worlds):
            act = self_mask[w] != 0
            ended = bool(((done[w] != 0) & (was[w] != 0)).any())
            restarted = bool((act & (was[w] == 0) & (done[w] == 0)).any())
            phase = int(st["phase"][w])
            armed = phase in (PREP, MAIN)
            if not act.any():
                table[BAD] += 1
            if ended and armed:                           # step 2
                main = phase == MAIN
                for kind, (base, o) in enumerate(((0, BOXES), (9, RAMPS))):
                    n = min(max(int(st["n_obj"][w, kind]), 0), (9, 2)[kind])
                    mp, mm, c = F(0), F(0), [0] * 6
                    for j in range(n):
                        e = base + j
                        s, p, l = st["start_pos"][w, e], st["prep_pos"][w, e], st["last_pos"][w, e]
                        move_prep = dist(p, s) if main else dist(l, s)
                        move_main = dist(l, p) if main else F(0)
                        mp, mm = np.fmax(mp, move_prep), np.fmax(mm, move_main)
                        le = int(st["last_locks"][w, e])
                        lp = int(st["prep_locks"][w, e]) if main else le
                        c[0] += bool(move_prep > eps); c[1] += bool(move_main > eps)
                        c[2] += lp == 1; c[3] += lp == 2; c[4] += le == 1; c[5] += le == 2
                    add(o + MAX_PREP, mp); add(o + MAX_MAIN, mm)
                    for q in range(6):
                        table[o + MOVED_PREP + q] += c[q]
                    table[o + OBJECTS] += n
                for side, o in ((0, SEEKERS), (1, HIDERS)):
                    add(o, st["travel"][w, side])
                    table[o + 1] += int(st["grab"][w, side]); table[o + 2] += int(st["agent_steps"][w, side])
                table[WORLD_EPISODES] += 1
                table[REACHED_MAIN] += main
            if act.any():
                first = int(np.argmax(act))
                p = int(prep_counter[w, first])
                hider = self_type[w] != 0
                steps = np.array([(act & ~hider).sum(), (act & hider).sum()], I)
                grab = np.array([(act & ~hider & (grabbing[w] != 0)).sum(), (act & hider & (grabbing[w] != 0)).sum()], I)
                if ended or phase == UNARMED or (phase != WAITING and restarted):         # step 3
                    nb, nr, nh = min(max(int(counts[w, 0]), 0), 9), min(max(int(counts[w, 1]), 0), 2), min(max(int(counts[w, 2]), 0), 6)
                    ns = min(max(int(counts[w, 3]), 0), 6 - nh)
                    st["n_obj"][w], st["n_side"][w] = (nb, nr), (ns, nh)
                    st["start_pos"][w], st["prep_pos"][w], st["last_pos"][w] = positions[w, :11], positions[w, :11], positions[w]
                    st["prep_locks"][w], st["last_locks"][w] = locks[w], locks[w]
                    st["travel"][w], st["grab"][w], st["agent_steps"][w] = F(0), grab, steps
                    st["phase"][w] = PREP if p > 0 else MAIN
                elif armed:                               # step 4
                    ns, nh = int(st["n_side"][w, 0]), int(st["n_side"][w, 1])
                    for i in range(6):
                        dd = dist(positions[w, 11 + i], st["last_pos"][w, 11 + i])
                        if i < nh:
                            st["travel"][w, 1] = F(st["travel"][w, 1] + dd)
                        elif i - nh < ns:
                            st["travel"][w, 0] = F(st["travel"][w, 0] + dd)
                    st["last_pos"][w], st["last_locks"][w] = positions[w], locks[w]
                    if phase == PREP and p == 0:
                        st["prep_pos"][w], st["prep_locks"][w], st["phase"][w] = positions[w, :11], locks[w], MAIN
                    st["grab"][w] += grab
                    st["agent_steps"][w] += steps
            was[w] = act                                  # step 6 (a view of the state)


def synthetic_calls(worlds, A, calls, seed=0):
    """A run to test on, a list of per-call input dicts.  Worlds whose episodes last 7 + w % 9 steps, staggered; with
    every episode a world draws its preparation length (0: the episode starts in the main phase; beyond the episode: it
    is cut before the seekers are released), how many boxes and ramps it has (0 included, and now and then a count out of
    range), how many of its rows are active (now and then none), how they split into hiders and seekers and whether the
    teams are flipped.  Positions drift, locks flip, agents grab.  As the simulator does it: done is written for the rows
    active in the episode that ends (the others keep what they had), everything else exported with a done is the next
    episode's.  Now and then a row joins in mid-episode with done = 0.  The first call's done is stale noise."""
    rng = np.random.default_rng([seed, worlds, A, calls])
    rows = worlds * A
    period = 7 + np.arange(worlds) % 9
    age = rng.integers(0, period)
    slot = np.tile(np.arange(A), worlds)

    def draw():
        active = np.where(rng.random(worlds) < 0.05, 0, rng.integers(1, A + 1, worlds))
        hiders = (rng.random(worlds) * (active + 1)).astype(np.int64)
        nb = np.where(rng.random(worlds) < 0.1, rng.choice(np.array([-3, 12, 100]), worlds), rng.integers(0, 10, worlds))
        nr = np.where(rng.random(worlds) < 0.1, rng.choice(np.array([-1, 3, 7]), worlds), rng.integers(0, 3, worlds))
        return active, hiders, nb, nr, rng.integers(0, 2, worlds), rng.integers(0, period + 3)
    active, hiders, nb, nr, flip, prep = draw()
    done = (rng.random(rows) < 0.3).astype(I)
    pos = (rng.standard_normal((worlds, 17, 2)) * 10).astype(F)
    locks = np.zeros((worlds, 11), I)
    out = []
    for _ in range(calls):
        age = age + 1
        over = age >= period
        mask_old = slot < np.repeat(active, A)
        done = np.where(mask_old, np.repeat(over, A).astype(I) * rng.choice(np.array([1, 7], I), rows), done).astype(I)
        na, nh, b, r, nf, npr = draw()
        join = ~over & (rng.random(worlds) < 0.03) & (active < A)
        joined = np.repeat(join, A) & (slot == np.repeat(active, A))
        done = np.where(joined, 0, done).astype(I)
        active = np.where(over, na, active + join)
        hiders, nb, nr, flip, prep = (np.where(over, x, y) for x, y in ((nh, hiders), (b, nb), (r, nr), (nf, flip), (npr, prep)))
        age = np.where(over, 0, age)
        mask = (slot < np.repeat(active, A)).astype(F)
        first = slot < np.repeat(hiders, A)               # the hiders first; flipped: the seekers first
        self_type = np.where(np.repeat(flip, A) == 1, ~first, first).astype(I)
        p = np.where(mask != 0, np.repeat(np.maximum(prep - age, 0), A), -5).astype(I)
        move = rng.random((worlds, 17, 1)) < 0.4
        pos = np.where(over[:, None, None], (rng.standard_normal((worlds, 17, 2)) * 10).astype(F),
                       np.where(move, pos + (rng.standard_normal((worlds, 17, 2)) * 0.4).astype(F), pos)).astype(F)
        locks = np.where(over[:, None], 0, np.where(rng.random((worlds, 11)) < 0.1, rng.integers(0, 3, (worlds, 11)), locks)).astype(I)
        seekers = np.clip(active - hiders, 0, None)
        counts = np.stack([nb, nr, hiders, seekers], 1).astype(I)
        grabbing = (rng.random(rows) < 0.3).astype(F)
        out.append(dict(positions=pos.copy(), locks=locks.copy(), counts=counts, prep_counter=p, done=done.copy(), self_type=self_type, self_mask=mask,
                        grabbing=grabbing))
    return out


def run(calls, worlds, A, phase=UNARMED, booked=None):
    st, table = new_state(worlds, A, phase), np.zeros(STATS)
    for c in calls:
        behaviour_step(st, table, A, **c, booked=booked)
    return st, table


def sum_bound(terms):
    """(n - 1) 2^-53 sum |x|, the bound of reordering an f64 sum of n terms, and the exact sum rounded once."""
    x = [float(v) for v in terms]
    return max(len(x) - 1, 0) * 2.0 ** -53 * sum(abs(v) for v in x), math.fsum(x)


# ---- properties of the restatement, one world of one hider (row 0) and one seeker (row 1), one box and one ramp ----
def _call(box=(0.0, 0.0), ramp=(5.0, 5.0), p=0, done=0, lock=0, mask=(1, 1), counts=(1, 1, 1, 1), hider=(1.0, 1.0), grab=(0, 0)):
    pos = np.zeros((1, 17, 2), F)
    pos[0, 0], pos[0, 9], pos[0, 11] = box, ramp, hider
    locks = np.zeros((1, 11), I)
    locks[0, 0] = lock
    return dict(positions=pos, locks=locks, counts=np.array([counts], I), prep_counter=np.array([p, p], I), done=np.array([done, done], I),
                self_type=np.array([1, 0], I), self_mask=np.array(mask, F), grabbing=np.array(grab, F))


def test_the_first_call_after_new_state_books_nothing_and_starts_an_episode():
    st, table = run([_call(p=3, done=1)], 1, 2)
    assert not table.any() and st["phase"][0] == PREP and st["was_active"].tolist() == [1, 1] and st["agent_steps"].tolist() == [[1, 1]]
    st, table = run([_call(p=0)], 1, 2)
    assert not table.any() and st["phase"][0] == MAIN


def test_a_box_moved_in_prep_shows_in_move_prep_alone_and_one_moved_after_in_move_main_alone():
    calls = [_call(p=2), _call(box=(3, 4), p=1), _call(box=(3, 4), p=0), _call(box=(3, 4), p=0), _call(done=1, p=2)]
    st, table = run(calls, 1, 2)
    assert table[WORLD_EPISODES] == 1 and table[REACHED_MAIN] == 1
    assert table[BOXES + MAX_PREP] == 5 and table[BOXES + MAX_MAIN] == 0 and table[BOXES + MOVED_PREP] == 1 and table[BOXES + MOVED_MAIN] == 0
    assert table[RAMPS + MAX_PREP] == 0 and table[RAMPS + OBJECTS] == 1 and table[BOXES + OBJECTS] == 1
    calls = [_call(p=1), _call(p=0), _call(box=(0, 0.25), p=0), _call(box=(6, 8), p=0), _call(done=1, p=2)]
    st, table = run(calls, 1, 2)
    assert table[BOXES + MAX_PREP] == 0 and table[BOXES + MAX_MAIN] == 10 and table[BOXES + MOVED_PREP] == 0 and table[BOXES + MOVED_MAIN] == 1
    # a displacement of move_eps itself is not "moved"
    st, table = run([_call(p=0), _call(box=(0, EPS), p=0), _call(done=1)], 1, 2)
    assert table[BOXES + MAX_MAIN] == EPS and table[BOXES + MOVED_MAIN] == 0


def test_a_lock_set_in_prep_and_released_in_main_counts_at_prep_end_only():
    calls = [_call(p=2), _call(p=1, lock=1), _call(p=0, lock=1), _call(p=0, lock=0), _call(done=1, p=2, lock=2)]
    st, table = run(calls, 1, 2)
    assert table[BOXES + HID_PREP] == 1 and table[BOXES + HID_END] == 0 and table[BOXES + SEEK_PREP] == 0 and table[BOXES + SEEK_END] == 0
    assert st["last_locks"][0, 0] == 2 and st["prep_locks"][0, 0] == 2        # the done call's lock is the next episode's
    calls = [_call(p=1), _call(p=0), _call(p=0, lock=2), _call(done=1, p=2)]
    st, table = run(calls, 1, 2)
    assert table[BOXES + SEEK_PREP] == 0 and table[BOXES + SEEK_END] == 1


def test_an_episode_cut_before_the_release_books_no_main_phase_and_its_locks_once():
    calls = [_call(p=5), _call(box=(3, 4), p=4, lock=1), _call(done=1, p=5)]
    st, table = run(calls, 1, 2)
    assert table[WORLD_EPISODES] == 1 and table[REACHED_MAIN] == 0
    assert table[BOXES + MAX_PREP] == 5 and table[BOXES + MAX_MAIN] == 0 and table[BOXES + MOVED_MAIN] == 0
    assert table[BOXES + HID_PREP] == 1 and table[BOXES + HID_END] == 1


def test_a_stale_done_on_a_row_that_left_books_nothing():
    calls = [_call(p=0, mask=(1, 0)), _call(p=0, mask=(1, 0), done=0)]
    calls[1]["done"] = np.array([0, 1], I)                # row 1 was never active
    calls.append(dict(calls[1]))
    st, table = run(calls, 1, 2)
    assert not table.any() and st["phase"][0] == MAIN and st["agent_steps"].tolist() == [[0, 3]]


def test_a_joining_row_restarts_the_world_without_booking():
    calls = [_call(p=0, mask=(1, 0)), _call(p=0, mask=(1, 0), hider=(4, 5)), _call(p=0, mask=(1, 1), hider=(7, 9))]
    st, table = run(calls, 1, 2)
    assert not table.any() and st["travel"].tolist() == [[0, 0]] and st["agent_steps"].tolist() == [[1, 1]]
    st, _ = run(calls[:2], 1, 2)
    assert st["travel"][0, 1] == 5 and st["travel"][0, 0] == 0
    # a waiting world does not start on it
    st, table = run(calls, 1, 2, phase=WAITING)
    assert not table.any() and st["phase"][0] == WAITING and not st["agent_steps"].any()


def test_a_waiting_world_starts_with_a_done_and_books_the_episode_after_it():
    calls = [_call(p=0), _call(p=0, done=1), _call(p=0, hider=(4, 5), grab=(1, 0)), _call(p=0, done=1)]
    st, table = run(calls, 1, 2, phase=WAITING)
    assert table[WORLD_EPISODES] == 1 and table[HIDERS] == 5 and table[HIDERS + 1] == 1 and table[HIDERS + 2] == 2 and table[SEEKERS + 2] == 2


def test_bad_counts_a_world_with_no_active_row_and_it_still_books():
    calls = [_call(p=0), _call(p=0, hider=(4, 5)), _call(p=0, done=1, mask=(0, 0)), _call(p=0, mask=(0, 0))]
    st, table = run(calls, 1, 2)
    assert table[BAD] == 2 and table[WORLD_EPISODES] == 1 and table[HIDERS] == 5
    assert st["phase"][0] == MAIN and st["was_active"].tolist() == [0, 0]     # no observation to start from: the state stands


def test_no_objects_give_plus_zero_maxima():
    calls = [_call(p=0, counts=(0, 0, 1, 1)), _call(box=(3, 4), ramp=(9, 9), p=0), _call(done=1)]
    st, table = run(calls, 1, 2)
    assert table[WORLD_EPISODES] == 1
    for o in (BOXES, RAMPS):
        assert not table[o:o + KIND].any() and not np.signbit(table[o:o + KIND]).any()


def test_counts_are_clamped_and_the_sides_take_their_own_entries():
    c = _call(p=0, counts=(100, -4, 9, 9))
    st, _ = run([c], 1, 2)
    assert st["n_obj"].tolist() == [[9, 0]] and st["n_side"].tolist() == [[0, 6]]
    a, b = _call(p=0, counts=(1, 1, 1, 1)), _call(p=0, counts=(1, 1, 1, 1), hider=(4, 5))
    b["positions"][0, 12] = (0, 2)                        # the seeker's entry follows the one hider's
    st, _ = run([a, b], 1, 2)
    assert st["travel"].tolist() == [[2, 5]]


def test_synthetic_run_covers_what_it_is_for():
    calls = synthetic_calls(13, 5, 300)
    booked = {}
    st, table = run(calls, 13, 5, booked=booked)
    assert table[WORLD_EPISODES] > 200 and 20 < table[REACHED_MAIN] < table[WORLD_EPISODES] - 20 and table[BAD] > 20
    assert table[BOXES + OBJECTS] > 500 and table[RAMPS + OBJECTS] > 100 and min(table[BOXES:SEEKERS]) > 0 and min(table[SEEKERS:]) > 0
    assert all(len(booked[i]) == table[WORLD_EPISODES] for i in F32_SUMS) and np.isfinite(table).all()
    stale = sum(int(((c["self_mask"] == 0) & (c["done"] != 0)).sum()) for c in calls)
    assert stale > 100 and any((c["counts"][:, 0] == 0).any() for c in calls) and any((c["counts"][:, 0] > 9).any() for c in calls)
    assert len({tuple(c["counts"][:, 2]) for c in calls}) > 10


# torch's vectorised CPU sqrt is within one ulp, not correctly rounded: a distance differs by 2^-23 relative at most, and a
# travel sum of n <= 16 x 6 of them (an episode of the synthetic run) by that plus n roundings of 2^-24 of the partial sums
SQRT_RTOL = (1 + 96) * 2.0 ** -23


def test_eager_step_equals_the_restatement_up_to_the_rounding_of_the_root():
    import torch
    from gpu_hideseek import behaviour as B
    worlds, A = 13, 5
    calls = synthetic_calls(worlds, A, 120)
    st, table = B.new_state(worlds, A, "cpu"), torch.zeros(STATS, dtype=torch.float64)
    want, want_table = new_state(worlds, A), np.zeros(STATS)
    for i, c in enumerate(calls):
        B.eager_step(st, table, A, *(torch.from_numpy(c[k]) for k in INPUTS), move_eps=EPS)
        behaviour_step(want, want_table, A, **c)
        for k in WORLD_KEYS + ROW_KEYS:
            if k == "travel":
                assert np.allclose(st[k].numpy(), want[k], rtol=SQRT_RTOL, atol=0), (i, k)
            else:
                assert np.array_equal(st[k].numpy().view(np.int32), want[k].view(np.int32)), (i, k)
    got = table.numpy()
    assert want_table[WORLD_EPISODES] > 50
    for i in range(STATS):
        if i in F32_SUMS:
            assert abs(got[i] - want_table[i]) <= SQRT_RTOL * want_table[i], (i, got[i], want_table[i])
        else:
            assert got[i] == want_table[i], (i, got[i], want_table[i])


# ---- request() ----
class _Sim:
    num_worlds, agents_per_world, gpu_id = 6, 4, 0


def test_request_refuses_before_the_library_is_called():
    import torch
    from gpu_hideseek import behaviour as B
    W, A = _Sim.num_worlds, _Sim.agents_per_world
    R = W * A
    i32 = torch.int32

    def call(state=None, table=None, **kw):
        st = B.new_state(W, A, "cpu")
        st.update(state or {})
        return B.compute(_Sim(), st, torch.zeros(B.STATS, dtype=torch.float64) if table is None else table, **kw)

    buf = torch.zeros(256, dtype=torch.float64)
    bad = [
        (dict(positions=torch.zeros(W, 17, 2, dtype=torch.float64)), "positions.*dtype"), (dict(positions=torch.zeros(W, 16, 2)), "positions.*shape"),
        (dict(locks=torch.zeros(W, 11)), "locks.*dtype"), (dict(locks=torch.zeros(W, 9, dtype=i32)), "locks.*shape"),
        (dict(counts=torch.zeros(W, 4, dtype=torch.int64)), "counts.*dtype"), (dict(counts=torch.zeros(W, 5, dtype=i32)), "counts.*shape"),
        (dict(prep_counter=torch.zeros(R)), "prep_counter.*dtype"), (dict(done=torch.zeros(A, W, dtype=i32)), "done.*shape"),
        (dict(self_type=torch.zeros(R, dtype=torch.int64)), "self_type.*dtype"), (dict(self_mask=torch.zeros(R, dtype=i32)), "self_mask.*dtype"),
        (dict(self_mask=torch.zeros(2 * R)[::2]), "self_mask.*not contiguous"), (dict(done=[0] * R), "done"),
        (dict(grabbing=torch.zeros(R, dtype=torch.float64)), "grabbing.*dtype"), (dict(grabbing=torch.zeros(R, 13)), "grabbing.*shape"),
        (dict(grabbing=torch.zeros(1).expand(R)), "grabbing.*stride"), (dict(grabbing=[0.0] * R), "grabbing"),
        (dict(state=dict(phase=torch.zeros(W + 1, dtype=i32))), "phase.*shape"), (dict(state=dict(last_pos=torch.zeros(W, 11, 2))), "last_pos.*shape"),
        (dict(state=dict(travel=torch.zeros(W, 2, dtype=i32))), "travel.*dtype"), (dict(state=dict(was_active=torch.zeros(W, dtype=i32))), "was_active.*shape"),
        (dict(state=dict(extra=torch.zeros(R))), "state must be"),
        (dict(table=torch.zeros(26, dtype=torch.float64)), "table.*shape"), (dict(table=torch.zeros(27)), "table.*dtype"),
        (dict(move_eps=float("nan")), "move_eps"), (dict(move_eps=float("inf")), "move_eps"), (dict(move_eps=-0.01), "move_eps"), (dict(move_eps=1e39), "move_eps"),
        (dict(state=dict(travel=buf.view(torch.float32)[:2 * W].view(W, 2)), table=buf[:27]), "table overlaps travel"),
        (dict(state=dict(grab=buf.view(i32)[4:4 + 2 * W].view(W, 2), agent_steps=buf.view(i32)[2 * W:4 * W].view(W, 2))), "agent_steps overlaps grab"),
        (dict(state=dict(start_pos=buf.view(torch.float32)[:22 * W].view(W, 11, 2)), positions=buf.view(torch.float32)[22 * W - 1:56 * W - 1].view(W, 17, 2)),
         "start_pos overlaps positions"),
        (dict(state=dict(was_active=buf.view(i32)[:R]), grabbing=buf.view(torch.float32)[R - 1:R - 1 + 13 * R:13]), "was_active overlaps grabbing"),
    ]
    for kw, what in bad:
        with pytest.raises(ValueError, match=what):
            call(**kw)
    # well formed, on the wrong device: every accepted form gets as far as the device check
    for shape in ((R,), (R, 1), (W, A)):
        with pytest.raises(ValueError, match="positions must be on cuda:0: it is on cpu"):
            call(positions=torch.zeros(W, 17, 2), locks=torch.zeros(W, 11, dtype=i32), counts=torch.zeros(W, 4, dtype=i32), prep_counter=torch.zeros(shape, dtype=i32),
                 done=torch.zeros(shape, dtype=i32), self_type=torch.zeros(shape, dtype=i32), self_mask=torch.zeros(shape), grabbing=torch.zeros(R, 13)[:, 12])
    with pytest.raises(ValueError, match="phase must be on cuda:0: it is on cpu"):
        call()
    with pytest.raises(ValueError, match="move_eps"):
        B.BehaviourStats(_Sim(), move_eps=-1.0)


# ---- stats_to_metrics ----
def test_stats_to_metrics_means_fractions_and_zero_for_empty_counts():
    import torch
    from gpu_hideseek import behaviour as B
    t = np.zeros(STATS)
    t[WORLD_EPISODES], t[REACHED_MAIN], t[BAD] = 4, 3, 2
    t[BOXES:BOXES + KIND] = [10.0, 6.0, 8, 4, 12, 2, 6, 1, 32]
    t[SEEKERS:SEEKERS + SIDE] = [50.0, 30, 200]
    for table in (torch.from_numpy(t), t.tolist()):
        m = B.stats_to_metrics(table)
        assert (m["world_episodes"], m["reached_main"], m["bad"]) == (4, 3, 2)
        b = m["boxes"]
        assert b["max_move_prep"] == 2.5 and b["max_move_main"] == 1.5 and b["moved_prep"] == 2 and b["moved_main"] == 1 and b["objects"] == 8
        assert b["hider_locked_prep"] == 3 and b["hider_locked_prep_fraction"] == 12 / 32 and b["seeker_locked_end_fraction"] == 1 / 32
        assert b["moved_prep_fraction"] == 0.25 and b["hider_locked_end"] == 1.5
        assert m["seekers"] == dict(agent_steps=200, travel_per_step=0.25, grab_rate=0.15)
        assert all(v == 0.0 for v in m["ramps"].values()) and all(v == 0.0 for v in m["hiders"].values())
    none = B.stats_to_metrics(torch.zeros(STATS, dtype=torch.float64))
    flat = [v for k in ("boxes", "ramps", "seekers", "hiders") for v in none[k].values()] + [none[k] for k in ("world_episodes", "reached_main", "bad")]
    assert len(flat) == 2 * 15 + 2 * 3 + 3 and all(v == 0.0 and not math.isnan(v) for v in flat)
    with pytest.raises(ValueError, match="table"):
        B.stats_to_metrics(torch.zeros(26))


# ---- the header ----
def test_header_mirror_and_symbols_agree(hideseek_lib):
    from gpu_hideseek import behaviour as B
    src = open(os.path.join(ROOT, "include", "hideseek.h")).read()
    flat = " ".join(src.split())
    assert "int32_t hs_behaviour_stats(hs_sim *sim, const hs_behaviour_request *req);" in flat
    assert "int32_t hs_behaviour_stats_async(hs_sim *sim, void *hip_stream, const hs_behaviour_request *req);" in flat
    enums = {k: int(v) for k, v in re.findall(r"(HS_BEHAVIOUR_[A-Z_]+) = (\d+)", src)}
    kind = {"HS_BEHAVIOUR_KIND_" + n.upper(): i for i, n in enumerate(B.KIND_NAMES)}
    side = {"HS_BEHAVIOUR_SIDE_" + n.upper(): i for i, n in enumerate(B.SIDE_NAMES)}
    assert enums == {"HS_BEHAVIOUR_STATS": 27, "HS_BEHAVIOUR_KIND_STATS": 9, "HS_BEHAVIOUR_SIDE_STATS": 3, "HS_BEHAVIOUR_UNARMED": 0, "HS_BEHAVIOUR_PREP": 1,
                     "HS_BEHAVIOUR_MAIN": 2, "HS_BEHAVIOUR_WAITING": 3, "HS_BEHAVIOUR_WORLD_EPISODES": 0, "HS_BEHAVIOUR_REACHED_MAIN": 1, "HS_BEHAVIOUR_BAD": 2,
                     "HS_BEHAVIOUR_BOXES": 3, "HS_BEHAVIOUR_RAMPS": 12, "HS_BEHAVIOUR_SEEKERS": 21, "HS_BEHAVIOUR_HIDERS": 24, **kind, **side}
    assert (B.STATS, B.KIND_STATS, B.SIDE_STATS) == (STATS, KIND, SIDE) and (B.UNARMED, B.PREP, B.MAIN, B.WAITING) == (UNARMED, PREP, MAIN, WAITING)
    assert (B.WORLD_EPISODES, B.REACHED_MAIN, B.BAD, B.BOXES, B.RAMPS, B.SEEKERS, B.HIDERS) == (0, 1, 2, 3, 12, 21, 24) and (B.SEEKER, B.HIDER) == (0, 1)
    assert B.RAMPS == B.BOXES + KIND and B.SEEKERS == B.RAMPS + KIND and B.HIDERS == B.SEEKERS + SIDE and B.STATS == B.HIDERS + SIDE
    body = re.search(r"typedef struct hs_behaviour_request \{(.*?)\} hs_behaviour_request;\s*/\* (\d+) bytes \*/", src, re.S)
    assert int(body.group(2)) == 176 == C.sizeof(B.HsBehaviourRequest)
    text = re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S)
    names = [n for decl in text.split(";") for n in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in B.HsBehaviourRequest._fields_]
    want = dict(positions=0, locks=8, counts=16, prep_counter=24, done=32, self_type=40, self_mask=48, grabbing=56, grab_stride=64, move_eps=68, phase=72,
                n_obj=80, n_side=88, start_pos=96, prep_pos=104, last_pos=112, prep_locks=120, last_locks=128, travel=136, grab=144, agent_steps=152,
                was_active=160, table=168)
    assert {n: getattr(B.HsBehaviourRequest, n).offset for n in want} == want
    assert list(B.STATE_KEYS) == names[10:22] == list(WORLD_KEYS + ROW_KEYS)
    L = C.CDLL(hideseek_lib)
    assert hasattr(L, "hs_behaviour_stats") and hasattr(L, "hs_behaviour_stats_async")
